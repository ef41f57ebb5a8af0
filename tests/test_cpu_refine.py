"""The edge split without a GPU: the two statements of tests/refine_mirror.py against each other on every mesh the GPU tests use, the
contract's rules asserted by hand, the Python checkers, the header and the command line's option errors."""
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
from rgbid import refine as RF
from rgbid import tsdf as TS
from tests import holes_mirror as HM
from tests import refine_mirror as RM
from tests.test_cpu_holes import attributes, join, mesh, punched
from tests.test_cpu_simplify import signed_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32, U8 = np.float32, np.uint32, np.uint8
NAN, INF = float("nan"), float("inf")
CUBE_LENGTHS = (0.2, 0.11, 0.05)
# what the mirror measured on the noisy cube over the three lengths: the largest relative change of the area and of
# the enclosed volume, in float64, between the input and the refined mesh; only the float32 rounding of the midpoints can move them
MEASURED_AREA, MEASURED_VOLUME = 7.6e-9, 3.7e-9


TRI = np.array([(0, 0, 0), (4, 0, 0), (0, 3, 0)], F)          # ab = 4, bc = 5, ca = 3


# ---- the meshes: name -> dict(vertices, triangles, colours, normals, selection, max_edge) ---------------------------------------------------
def case(m, max_edge, selection=None):
    return dict(m, selection=None if selection is None else np.array(selection, U8).reshape(-1), max_edge=float(max_edge))


def cube(n=4, noise=0.0, seed=11):
    """the unit cube with n cells per edge, every cell cut along the same diagonal, outward orientation; float32 positions with seeded
    normal noise"""
    index, pts, tris = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(pts)
            pts.append(p)
        return index[p]

    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    def corner(da, db):
                        q = [0, 0, 0]
                        q[axis], q[u], q[v] = side, a + da, b + db
                        return vid(tuple(q))
                    p00, p10, p11, p01 = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    outward = (side == n) == (axis != 1)
                    for t in ((p00, p10, p11), (p00, p11, p01)):
                        tris.append(t if outward else t[::-1])
    pos = np.array(pts, np.float64) / n
    if noise:
        pos = pos + np.random.default_rng(seed).normal(0.0, noise, pos.shape)
    return mesh(pos.astype(F), tris)


def fan_in_strip(k=64, rim=1.0, outer=1.25):
    """a fan of k triangles around the hub 0 (rim vertices 1 .. k) inside a strip of 2 k triangles out to the vertices k + 1 .. 2 k; the
    first k triangles are the fan"""
    ang = 2.0 * np.pi * np.arange(k) / k
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(k)], 1)
    pos = np.concatenate([[[0.0, 0.0, 0.0]], rim * ring, outer * ring])
    i = np.arange(k)
    j = (i + 1) % k
    fan = np.stack([np.zeros(k, np.int64), 1 + i, 1 + j], 1)
    strip = np.concatenate([np.stack([1 + i, 1 + k + i, 1 + k + j], 1), np.stack([1 + i, 1 + k + j, 1 + j], 1)])
    return mesh(pos, np.concatenate([fan, strip]))


def grid(nx, ny, seed=None):
    """a sheet of nx x ny cells in the plane z = 0, two triangles per cell, unit cells; with a seed the positions are jittered"""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    pos = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size)], 1).astype(np.float64)
    if seed is not None:
        pos += np.random.default_rng(seed).uniform(-0.2, 0.2, pos.shape)
    vid = lambda a, b: a * (ny + 1) + b
    a, b = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    tri = np.concatenate([np.stack([vid(a, b), vid(a + 1, b), vid(a + 1, b + 1)], 1), np.stack([vid(a, b), vid(a + 1, b + 1), vid(a, b + 1)], 1)])
    return mesh(pos, tri)


def hand_mesh():
    """every rule on a few vertices; max_edge = 1.5"""
    flat = lambda pts: [(x, y, 0) for x, y in pts]
    parts = [mesh(flat([(0, 0), (2, 0), (0, 1)]), [(0, 1, 2)]),                                  # 0 - 2: ab and bc marked (2, sqrt 5), ca not
             mesh(flat([(10, 0), (12, 0), (10, 2), (12, 2)]), [(0, 1, 2), (1, 3, 2)]),            # 3 - 6: all edges marked, 4 5 shared
             mesh(flat([(20, 0), (22, 0), (21, 1), (21, -1), (21, 0.5)]), [(0, 1, 2), (1, 0, 3), (0, 1, 4), (0, 1, 2)]),   # 7 - 11: 7 8 in four
             mesh(flat([(30, 0), (35, 0), (30, 5)]), [(0, 0, 1), (2, 2, 2), (1, 2, 1)]),          # 12 - 14: repeated indices only
             mesh([(NAN, 0, 0), (42, 0, 0), (40, 2, 0)], [(0, 1, 2)]),                            # 15 - 17: a NaN: only 16 17 can be marked
             mesh([(50, 0, 0), (52, -INF, 0), (50, 2, 0)], [(0, 1, 2)]),                          # 18 - 20: an inf: only 20 18 can be marked
             mesh(flat([(60, 0), (61, 0), (60, 1)]), [(0, 1, 2)]),                                # 21 - 23: nothing above 1.5
             mesh(flat([(70, 0), (73, 0), (70, 1)]), [(0, 1, 2), (1, 0, 2)])]                     # 24 - 26: both orientations
    m, first = join(*parts)
    assert first == [0, 3, 7, 12, 15, 18, 21, 24]
    v = m["vertices"].view(U32)
    v[17, 2] = 0x7F800001                                                                         # a signalling NaN: 16 17 is not marked either
    col = np.full((len(v), 3), 9, U8)
    col[0:3] = [(254, 0, 7), (255, 1, 8), (0, 0, 0)]
    nrm = np.tile(np.array([0, 0, 1], F), (len(v), 1))
    nrm[3:5] = [(1, 0, 0), (-1, 0, 0)]                                                            # they cancel on the edge 3 4
    return dict(m, colours=col, normals=nrm)


def diagonal_mesh(x, y):
    """the triangle (0, 1, 2) with a = (0, 0), b = (2 x, 0), c = (2 x, 2 y) and a neighbour across ab and across bc: with the selection
    0 1 1 and L = 0 exactly ab and bc are marked in it, m0 = (x, 0), m1 = (2 x, y), q(m0, c) = x^2 + 4 y^2, q(a, m1) = 4 x^2 + y^2: m0 - c
    is the shorter one iff y < x, and they are equal iff y = x"""
    return mesh([(0, 0, 0), (2 * x, 0, 0), (2 * x, 2 * y, 0), (x, -1, 0), (2 * x + 1, y, 0)], [(0, 1, 2), (1, 0, 3), (2, 1, 4)])


DIAGONALS = {"diagonal_m0c": (2.0, 1.0), "diagonal_am1": (1.0, 2.0), "diagonal_tie": (1.5, 1.5)}
# coordinates whose float32 sum overflows while their midpoint does not: the midpoint is formed in double
HUGE = mesh([(3e38, 0, 0), (3.2e38, 1, 0), (3.1e38, -3e38, 2)], [(0, 1, 2)])


def random_soup(n_v, n_t, seed):
    """random triangles over few vertices: duplicates, repeated indices and edges in many triangles"""
    rng = np.random.default_rng(seed)
    return mesh(rng.uniform(-1, 1, (n_v, 3)).astype(F), rng.integers(0, n_v, (n_t, 3)))


def median_edge(m):
    p = m["vertices"].astype(np.float64)[m["triangles"].astype(np.int64)]
    ok = np.isfinite(p).all((1, 2))
    return float(np.median(np.sqrt(((p[ok] - p[ok][:, (1, 2, 0)]) ** 2).sum(2))))


@functools.lru_cache(maxsize=None)
def all_cases():
    fan = fan_in_strip()
    soup = random_soup(40, 600, 5)
    cases = {"hand": case(hand_mesh(), 1.5), "hand_every_edge": case(hand_mesh(), 0.0), "hand_nothing": case(hand_mesh(), 1e6),
             "hand_selected": case(hand_mesh(), 1.5, [1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 0]),
             "no_triangles": case(mesh([(0.1, 0.2, 0.3), (4, 5, 6), (NAN, 1, 2)], []), 0.1), "no_vertices": case(mesh([], []), 0.1),
             "fan_only": case(fan, 0.15, [1] * 64 + [0] * 128), "fan_all": case(fan, 0.1), "soup": case(soup, median_edge(soup)),
             "soup_third": case(soup, 0.5 * median_edge(soup), (np.arange(600) % 3 == 0) * 255),
             "grid_jitter": case(grid(9, 7, 3), 1.1), "cube_clean_every_edge": case(cube(), 0.0),
             "exactly_the_length": case(mesh(TRI, [(0, 1, 2)]), 4.0), "huge": case(HUGE, 0.0)}
    for name, (x, y) in DIAGONALS.items():
        cases[name] = case(diagonal_mesh(x, y), 0.0, [0, 1, 1])
    for L in CUBE_LENGTHS:
        cases[f"cube_{L}"] = case(cube(noise=0.03), L)
    for seed, (name, m) in enumerate(sorted(cases.items())):
        if m["colours"] is None:
            m["colours"], m["normals"] = attributes(len(m["vertices"]), seed)
    return cases


@functools.lru_cache(maxsize=None)
def planned(name):
    """the vectorised mirror's plan of a case, computed once and shared with the GPU tests"""
    m = all_cases()[name]
    return RM.plan(m["triangles"], m["vertices"], m["max_edge"], m["selection"])


@functools.lru_cache(maxsize=None)
def emitted(name):
    """-> (vertices, colours, normals, triangles, selection) of one round; the selection is written out even where the case has none"""
    m = all_cases()[name]
    sel = np.ones(len(m["triangles"]), U8) if m["selection"] is None else m["selection"]
    return RM.emit(planned(name), m["vertices"], m["colours"], m["normals"], sel)


@functools.lru_cache(maxsize=None)
def refined(name, rounds=8):
    m = all_cases()[name]
    return RM.refine(m["vertices"], m["colours"], m["triangles"], m["normals"], m["max_edge"], rounds, m["selection"])


# ---- the two statements ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_mirror_equals_the_loops(name):
    m = all_cases()[name]
    table = RM.plan_loop(m["triangles"], m["vertices"], m["max_edge"], m["selection"])
    assert RM.same_table(planned(name), table) == []
    c = table["counts"]
    assert c["k0"] + c["k1"] + c["k2"] + c["k3"] == len(m["triangles"]) and c["new_triangles"] == c["k1"] + 2 * c["k2"] + 3 * c["k3"]
    assert c["marked"] <= c["eligible"] <= c["edges"] <= 3 * (len(m["triangles"]) - c["degenerate"])
    sel = np.ones(len(m["triangles"]), U8) if m["selection"] is None else m["selection"]
    assert RM.same(emitted(name), RM.emit_loop(table, m["vertices"], m["colours"], m["normals"], sel)) == []
    v, col, nrm, t, s = emitted(name)
    assert len(v) == len(col) == len(nrm) == len(m["vertices"]) + c["marked"] and len(t) == len(s) == len(m["triangles"]) + c["new_triangles"]
    assert v[:len(m["vertices"])].tobytes() == m["vertices"].tobytes() and nrm[:len(m["vertices"])].tobytes() == m["normals"].tobytes()


@pytest.mark.parametrize("name", ["hand", "hand_selected", "fan_only", "soup", "cube_0.11"])
def test_rounds_of_both_statements(name):
    m = all_cases()[name]
    a = refined(name, 3)
    b = RM.refine(m["vertices"], m["colours"], m["triangles"], m["normals"], m["max_edge"], 3, m["selection"], loop=True)
    assert RM.same((a[0], a[1], a[3], a[2], a[4]), (b[0], b[1], b[3], b[2], b[4])) == [] and a[5] == b[5]


def test_one_shot_without_attributes():
    m = all_cases()["cube_0.11"]
    v, c, t, n, s, fig = RM.refine(m["vertices"], None, m["triangles"], None, 0.11, 8)
    full = refined("cube_0.11")
    assert c is None and n is None and v.tobytes() == full[0].tobytes() and t.tobytes() == full[2].tobytes() and fig == full[5]


# ---- the split patterns by hand ------------------------------------------------------------------------------------------------------------


def one_triangle(rot, max_edge, pos=TRI):
    """the triangle (a, b, c) named from corner `rot` on -> (table, output triangles as lists, the names a b c of the rows)"""
    names = [(0, 1, 2), (1, 2, 0), (2, 0, 1)][rot]
    table = RM.plan([names], pos, max_edge)
    return table, RM.emit(table, pos)[3].tolist(), RM.emit(table, pos)[0]


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_pattern_k0_and_k3(rot):
    a, b, c = [(0, 1, 2), (1, 2, 0), (2, 0, 1)][rot]
    table, rows, v = one_triangle(rot, 5.0)
    assert table["counts"] == dict(edges=3, eligible=3, marked=0, k0=1, k1=0, k2=0, k3=0, degenerate=0, new_triangles=0) and rows == [[a, b, c]]
    table, rows, v = one_triangle(rot, 2.9)
    assert table["counts"] == dict(edges=3, eligible=3, marked=3, k0=0, k1=0, k2=0, k3=1, degenerate=0, new_triangles=3)
    # the edges in (lo, hi) order are 01, 02, 12 -> the vertices 3, 4, 5
    new = {(0, 1): 3, (0, 2): 4, (1, 2): 5}
    m0, m1, m2 = (new[tuple(sorted(e))] for e in ((a, b), (b, c), (c, a)))
    assert rows == [[a, m0, m2], [m0, b, m1], [m2, m1, c], [m0, m1, m2]]
    assert v[3].tolist() == [2, 0, 0] and v[4].tolist() == [0, 1.5, 0] and v[5].tolist() == [2, 1.5, 0]


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_pattern_k1(rot):
    a, b, c = [(0, 1, 2), (1, 2, 0), (2, 0, 1)][rot]
    table, rows, v = one_triangle(rot, 4.5)                    # only the edge 1 2 of length 5
    assert table["counts"]["marked"] == 1 and table["counts"]["k1"] == 1 and v[3].tolist() == [2, 1.5, 0]
    # rotated so that 1 2 is ab: (1, 2, 0) whatever the triangle's first corner
    assert rows == [[1, 3, 0], [3, 2, 0]]


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_pattern_k2_and_its_diagonal(rot):
    names = [(0, 1, 2), (1, 2, 0), (2, 0, 1)][rot]
    table, rows, v = one_triangle(rot, 3.5)                    # 0 1 and 1 2 are marked, 2 0 is not: rotated to (a, b, c) = (0, 1, 2)
    assert table["counts"]["marked"] == 2 and table["counts"]["k2"] == 1 and names
    m0, m1 = 3, 4                                              # on 0 1 and on 1 2
    assert v[3].tolist() == [2, 0, 0] and v[4].tolist() == [2, 1.5, 0]
    # q(m0, c) = 4 + 9 = 13, q(a, m1) = 4 + 2.25 = 6.25: not smaller, the cut runs along a - m1
    assert rows == [[m0, 1, m1], [0, m0, m1], [0, m1, 2]]
    tall = np.array([(0, 0, 0), (4, 0, 0), (3, 1, 0)], F)      # ab = 4, bc = sqrt 2, ca = sqrt 10: mark ab and ca with 2 < L < 3.16
    table = RM.plan([names], tall, 2.0)
    assert table["counts"]["k2"] == 1
    v, _, _, t, _ = RM.emit(table, tall)
    # 1 2 is unmarked: rotated to (a, b, c) = (2, 0, 1), m0 on 2 0 (vertex 4: edges 01 -> 3, 02 -> 4), m1 on 0 1 (vertex 3)
    # q(m0, c) = |(1.5, .5) - (4, 0)|^2 = 6.5, q(a, m1) = |(3, 1) - (2, 0)|^2 = 2: along a - m1
    assert t.tolist() == [[4, 0, 3], [2, 4, 3], [2, 3, 1]]


@pytest.mark.parametrize("name, along_m0c", [("diagonal_m0c", True), ("diagonal_am1", False), ("diagonal_tie", False)])
def test_diagonal_both_ways_and_the_tie(name, along_m0c):
    x, y = DIAGONALS[name]
    table = planned(name)
    assert table["edges"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [1, 4], [2, 4]] and table["rank"].tolist() == [0, -1, 1, 2, 3, 4, 5]
    assert table["k"].tolist() == [2, 3, 3] and table["eligible"].tolist() == [True, False, True, True, True, True, True]
    v, _, _, t, sel = emitted(name)
    assert v[5].tolist() == [x, 0, 0] and v[7].tolist() == [2 * x, y, 0]
    q = lambda a, b: float(((v[a].astype(np.float64) - v[b].astype(np.float64)) ** 2).sum())
    assert (q(5, 2) < q(0, 7)) == along_m0c and (q(5, 2) == q(0, 7)) == (name == "diagonal_tie")
    rows = t.tolist()
    assert rows[0] == [5, 1, 7] and rows[3:5] == ([[0, 5, 2], [5, 7, 2]] if along_m0c else [[0, 5, 7], [0, 7, 2]])
    assert sel.tolist() == [0, 1, 1, 0, 0] + [1] * 6


def test_a_length_that_an_edge_has_exactly_and_a_sum_beyond_float32():
    table = planned("exactly_the_length")                          # q = 16 = L L for ab: not above it
    assert table["counts"]["marked"] == 1 and table["rank"].tolist() == [-1, -1, 0] and emitted("exactly_the_length")[3].tolist() == [[1, 3, 0], [3, 2, 0]]
    m = all_cases()["huge"]
    with np.errstate(over="ignore"):
        assert np.isinf(m["vertices"][0] + m["vertices"][1]).any()   # the float32 sum is infinite ...
    v = emitted("huge")[0]
    assert planned("huge")["counts"]["marked"] == 3 and np.isfinite(v).all()     # ... the midpoint is not
    assert v[3].tolist() == [F(3.1e38), 0.5, 0] and v[3, 0] == F((float(m["vertices"][0, 0]) + float(m["vertices"][1, 0])) / 2.0)


def test_shared_and_non_manifold_edges_get_one_midpoint():
    v, c, n, t, s = emitted("hand")
    m = all_cases()["hand"]
    table = planned("hand")
    # the pair 3 - 6: five distinct edges, all marked, the shared edge 4 5 once
    pair = [e for e, (lo, hi) in enumerate(table["edges"].tolist()) if 3 <= lo <= 6]
    assert len(pair) == 5 and all(table["rank"][e] >= 0 for e in pair)
    mid45 = len(m["vertices"]) + int(table["rank"][table["edges"].tolist().index([4, 5])])
    rows = t.tolist()
    assert sum(mid45 in r for r in rows) == 6                    # three children of each of the two triangles
    # 7 8 is named by four triangles (one given twice): one edge, one midpoint, in every one of them
    e78 = table["edges"].tolist().index([7, 8])
    assert (table["corner_edge"][3:7] == e78).sum() == 4 and table["rank"][e78] >= 0
    mid78 = len(m["vertices"]) + int(table["rank"][e78])
    assert v[mid78].tolist() == [21, 0, 0]
    assert rows[3] == rows[6] and all(mid78 in rows[i] for i in (3, 4, 5, 6))


def test_triangles_left_alone():
    m, table = all_cases()["hand"], planned("hand")
    v, c, n, t, s = emitted("hand")
    rows = t.tolist()
    assert table["counts"]["degenerate"] == 3 and (table["corner_edge"][7:10] == -1).all() and rows[7:10] == [[12, 12, 13], [14, 14, 14], [13, 14, 13]]
    assert not any(lo in (12, 13, 14) for lo, hi in table["edges"].tolist())
    # the NaN triangle (15 16 17 with a signalling NaN in 17 too): no edge is marked, the words are kept
    assert table["k"][10] == 0 and rows[10] == [15, 16, 17]
    assert v[:len(m["vertices"])].tobytes() == m["vertices"].tobytes() and v.view(U32)[17, 2] == 0x7F800001
    # the inf triangle (18 19 20): 20 18 has length 2 and is marked, the two edges at 19 are not
    assert table["k"][11] == 1 and rows[11] == [20, len(m["vertices"]) + int(table["rank"][table["edges"].tolist().index([18, 20])]), 19]
    assert table["k"][12] == 0 and rows[12] == [21, 22, 23]
    # both orientations of one triangle keep theirs
    area_z = lambda r: float(np.cross(v[r[1]] - v[r[0]], v[r[2]] - v[r[0]])[2])
    kids = lambda i: [rows[i]] + rows[len(m["triangles"]) + table["base"][i]:len(m["triangles"]) + table["base"][i] + table["k"][i]]
    assert all(area_z(r) > 0 for r in kids(13)) and all(area_z(r) < 0 for r in kids(14)) and table["k"][13] == table["k"][14] == 2
    assert abs(sum(area_z(r) for r in kids(13)) - 3.0) < 1e-6


def test_attributes():
    m, table = all_cases()["hand"], planned("hand")
    v, c, n, t, s = emitted("hand")
    n_v = len(m["vertices"])
    r01 = n_v + int(table["rank"][table["edges"].tolist().index([0, 1])])
    assert c[r01].tolist() == [255, 1, 8]                        # (254 + 255 + 1) >> 1, (0 + 1 + 1) >> 1, (7 + 8 + 1) >> 1
    r34 = n_v + int(table["rank"][table["edges"].tolist().index([3, 4])])
    assert n[r34].tolist() == [0, 0, 0]                          # opposite normals
    r56 = n_v + int(table["rank"][table["edges"].tolist().index([5, 6])])
    assert n[r56].tolist() == [0, 0, 1]


def test_extreme_lengths():
    m = all_cases()["cube_clean_every_edge"]
    c = planned("cube_clean_every_edge")["counts"]
    assert c["edges"] == c["marked"] == 288 and c["k3"] == 192 and len(emitted("cube_clean_every_edge")[3]) == 4 * 192
    c = planned("hand_every_edge")["counts"]
    # every edge whose ends are finite: the NaN triangle has none, the inf triangle one
    assert c["marked"] == c["edges"] - 3 - 2
    h = all_cases()["hand_nothing"]
    assert planned("hand_nothing")["counts"]["marked"] == 0
    v, col, nrm, t, s = emitted("hand_nothing")
    assert v.tobytes() == h["vertices"].tobytes() and t.tobytes() == h["triangles"].tobytes() and col.tobytes() == h["colours"].tobytes()
    with pytest.raises(ValueError):
        RM.plan(m["triangles"], m["vertices"], -1.0)
    for bad in (NAN, INF, -INF):
        with pytest.raises(ValueError):
            RM.plan(m["triangles"], m["vertices"], bad)


def test_selection():
    m, table = all_cases()["hand_selected"], planned("hand_selected")
    full = planned("hand")
    edges = table["edges"].tolist()
    assert edges == full["edges"].tolist() and table["counts"]["eligible"] < full["counts"]["eligible"]
    # triangle 1 (3 4 5) is selected, triangle 2 (4 6 5) is not: 4 5, 3 4, 3 5 split, 4 6 and 5 6 do not, triangle 2 is cut with k = 1
    assert table["k"][1] == 3 and table["k"][2] == 1
    assert table["rank"][edges.index([4, 6])] == -1 and table["rank"][edges.index([5, 6])] == -1 and not table["eligible"][edges.index([4, 6])]
    v, c, n, t, s = emitted("hand_selected")
    n_t = len(m["triangles"])
    assert s[:n_t].tobytes() == m["selection"].tobytes()
    for i in range(n_t):
        assert (s[n_t + table["base"][i]:n_t + table["base"][i] + table["k"][i]] == m["selection"][i]).all()
    third = all_cases()["soup_third"]
    assert set(np.unique(emitted("soup_third")[4]).tolist()) == {0, 255} and (third["selection"] != 0).sum() == 200


def test_all_four_patterns_occur_in_the_soup():
    c = planned("soup")["counts"]
    assert min(c["k0"], c["k1"], c["k2"], c["k3"]) > 0 and c["degenerate"] > 0 and c["edges"] < 3 * 600


# ---- many rounds -----------------------------------------------------------------------------------------------------------------------------
def euler(tri):
    t = tri.astype(np.int64)
    e = np.unique(np.sort(np.stack([t, t[:, (1, 2, 0)]], 2).reshape(-1, 2), 1), axis=0)
    return len(np.unique(t)) - len(e) + len(t)


def area(v, tri):
    p = v.astype(np.float64)[tri.astype(np.int64)]
    return float(np.sqrt((np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) ** 2).sum(1)).sum() / 2.0)


def longest_edge(v, tri):
    p = v.astype(np.float64)[tri.astype(np.int64)]
    return float(np.sqrt(((p - p[:, (1, 2, 0)]) ** 2).sum(2)).max())


@pytest.mark.parametrize("L, rounds_needed", [(0.2, 2), (0.11, 3), (0.05, 4)])
def test_noisy_cube(L, rounds_needed):
    m = all_cases()[f"cube_{L}"]
    assert m["vertices"].shape == (98, 3) and m["triangles"].shape == (192, 3)
    v, c, t, n, s, fig = refined(f"cube_{L}")
    print(f"L = {L}: {fig['rounds_run']} rounds, {len(v)} vertices, {len(t)} triangles, longest edge {longest_edge(v, t):.4f}")
    assert fig["left"] == 0 and fig["rounds_run"] == rounds_needed and longest_edge(v, t) <= L
    assert euler(m["triangles"]) == 2 and euler(t) == 2
    assert HM.plan(m["triangles"], 98)["counts"]["boundary_half_edges"] == 0 and HM.plan(t, len(v))["counts"]["boundary_half_edges"] == 0
    a0, a1, v0, v1 = area(m["vertices"], m["triangles"]), area(v, t), signed_volume(m["vertices"], m["triangles"]), signed_volume(v, t)
    print(f"  area {a0!r} -> {a1!r} ({abs(a1 - a0) / a0:.3g}), volume {v0!r} -> {v1!r} ({abs(v1 - v0) / v0:.3g})")
    assert abs(a1 - a0) <= 10 * MEASURED_AREA * a0 and abs(v1 - v0) <= 10 * MEASURED_VOLUME * v0 and v0 > 0


def test_fan_in_strip():
    m = all_cases()["fan_only"]
    v, c, t, n, s, fig = refined("fan_only")
    assert fig["left"] == 0 and fig["rounds_run"] >= 2
    before, after = HM.plan(m["triangles"], len(m["vertices"]))["counts"], HM.plan(t, len(v))["counts"]
    assert before["boundary_half_edges"] == after["boundary_half_edges"] == 64 and after["loops"] == 1
    sel = s != 0
    p = v.astype(np.float64)[t.astype(np.int64)]
    assert np.sqrt(((p - p[:, (1, 2, 0)]) ** 2).sum(2))[sel].max() <= 0.15 and sel.sum() > 64 and abs(area(v, t) - area(m["vertices"], m["triangles"])) < 1e-6
    assert refined("fan_all")[5]["left"] == 0


def test_open_cube_caps_only():
    whole = cube(noise=0.03)
    centre = int(np.flatnonzero((np.abs(cube()["vertices"] - np.array([0.5, 0.5, 1.0], F)) < 1e-6).all(1))[0])
    m, removed = punched(whole, [centre])
    col, nrm = attributes(98, 77)
    fv, fc, ft, fn, fig = HM.fill(m["vertices"], col, m["triangles"], nrm, 16)
    n_in = len(m["triangles"])
    assert removed == 6 and fig["filled"] == 1 and len(ft) == n_in + 6
    sel = np.zeros(len(ft), U8)
    sel[n_in:] = 1
    v, c, t, n, s, figures = RM.refine(fv, fc, ft, fn, 0.11, 8, sel)
    assert figures["left"] == 0 and figures["rounds_run"] >= 1 and len(t) > len(ft)
    key = lambda tri: (np.minimum(tri, tri[:, (1, 2, 0)]).astype(np.int64) << 32) | np.maximum(tri, tri[:, (1, 2, 0)]).astype(np.int64)
    cap_edges = np.unique(key(ft[n_in:]))
    apart = ~np.isin(key(ft[:n_in]), cap_edges).any(1)
    assert 0 < apart.sum() < n_in
    assert t[:n_in][apart].tobytes() == ft[:n_in][apart].tobytes() and v[:len(fv)].tobytes() == fv.tobytes() and (s[:n_in] == 0).all()
    assert HM.plan(t, len(v))["counts"]["boundary_half_edges"] == 0 and euler(t) == 2


def test_empty_meshes_and_no_rounds():
    for name in ("no_triangles", "no_vertices"):
        m = all_cases()[name]
        assert planned(name)["counts"] == dict.fromkeys(RM.PLAN_COUNTS, 0)
        v, c, n, t, s = emitted(name)
        assert v.tobytes() == m["vertices"].tobytes() and t.shape == (0, 3) and s.shape == (0,)
    m = all_cases()["hand"]
    v, c, t, n, s, fig = RM.refine(m["vertices"], m["colours"], m["triangles"], m["normals"], 1.5, 0)
    assert fig == dict(rounds=[], rounds_run=0, left=planned("hand")["counts"]["marked"]) and t.tobytes() == m["triangles"].tobytes()
    for r in (-1, 17, 1.5, True):
        with pytest.raises(ValueError):
            RM.refine(m["vertices"], None, m["triangles"], None, 1.5, r)
    with pytest.raises(ValueError):
        RM.plan([(0, 1, 3)], m["vertices"][:3], 1.0)


# ---- the Python checkers, one by one ------------------------------------------------------------------------------------------------------
def test_checkers():
    assert RF.capacity_arg(1, 1) == (1, 1) and RF.capacity_arg(1 << 31, np.int64(1 << 29)) == (1 << 31, 1 << 29)
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 1), (1, (1 << 29) + 1), (-1, 1), (1.0, 1), (1, "1"), (None, 1), (True, 1)):
        with pytest.raises(ValueError):
            RF.capacity_arg(v, t)
    assert RF.max_edge_arg(0) == 0.0 and RF.max_edge_arg(np.float32(0.5)) == 0.5 and RF.max_edge_arg(3) == 3.0
    for bad in (-1e-9, NAN, INF, -INF, "0.1", None, True):
        with pytest.raises(ValueError):
            RF.max_edge_arg(bad)
    assert RF.rounds_arg(0) == 0 and RF.rounds_arg(np.int64(16)) == 16
    for bad in (-1, 17, 4.0, "4", None, True):
        with pytest.raises(ValueError):
            RF.rounds_arg(bad)
    assert RF.refine_arg(None) is None and RF.refine_arg(0.05) == dict(max_edge=0.05, rounds=4, caps_only=False)
    assert RF.refine_arg(dict(max_edge=1, rounds=0, caps_only=True)) == dict(max_edge=1.0, rounds=0, caps_only=True)
    for bad in (-0.1, NAN, "0.1", dict(rounds=2), dict(max_edge=0.1, round=2), dict(max_edge=0.1, caps_only=1), dict(max_edge=0.1, rounds=17)):
        with pytest.raises(ValueError):
            RF.refine_arg(bad)
    assert RF.PLAN_COUNTS == RM.PLAN_COUNTS and RF.MAX_ROUNDS == RM.MAX_ROUNDS == 16


def test_tensor_checkers_need_cuda_tensors():
    import torch
    ht = torch.zeros((4, 3), dtype=torch.int32)
    for t, n in ((ht, 5), (ht.numpy(), 5), (None, 5)):
        with pytest.raises(ValueError):
            RF.mesh_arg(t, n)
    hv = torch.zeros((4, 3), dtype=torch.float32)
    for args in ((hv, None, None, 4), (None, None, None, 0), (hv.numpy(), None, None, 4)):
        with pytest.raises(ValueError):
            RF.attributes_arg(*args)
    assert RF.selection_arg(None, 4) is None
    for s in (torch.zeros(4, dtype=torch.uint8), np.zeros(4, U8), [1, 0, 1, 0]):
        with pytest.raises(ValueError):
            RF.selection_arg(s, 4)


def test_checks_come_before_the_library():
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 4), (4, (1 << 29) + 1)):
        with pytest.raises(ValueError):
            RF.Refiner(None, v, t)

    class Ctx:
        device = 0
    rf = RF.Refiner.__new__(RF.Refiner)
    rf.ctx, rf.max_vertices, rf.max_triangles, rf.counts, rf.n_vertices, rf.n_triangles = Ctx(), 10, 10, None, 0, 0
    for L in (-1.0, NAN, "1"):
        with pytest.raises(ValueError):
            rf.plan(None, None, L)
    with pytest.raises(ValueError):
        rf.plan(np.zeros((1, 3), np.int32), np.zeros((3, 3), F), 1.0)
    with pytest.raises(ValueError):
        rf.emit(None, None)                                         # nothing is planned
    rf._h = None
    for L, r in ((-1.0, 4), (0.1, 17), (0.1, 2.0), (NAN, 1)):
        with pytest.raises(ValueError):
            RF.refine_mesh(None, None, None, None, None, L, r)
    with pytest.raises(ValueError):
        RF.refine_mesh(None, None, None, None, None, 0.1)           # no tensors
    kf = [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)]
    for f in (-1.0, "x", dict(rounds=3), dict(max_edge=0.1, caps_only=True), dict(max_edge=0.1, rounds=-1)):
        with pytest.raises(ValueError):
            TS.fuse(None, kf, (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), refine=f)
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels = Ctx(), 2, 1000
    for f in (-1.0, dict(max_edge=INF), dict(max_edge=0.1, caps_only=True)):
        with pytest.raises(ValueError):
            vol.extract(1, refine=f)
    vol._h = None


def test_nothing_is_imported_without_the_option():
    """fuse checks its options before it looks at the keyframes: without refine the module is not imported, with it it is"""
    code = ("import sys, inspect; sys.path[:0] = [%r, %r]; from rgbid import tsdf as TS\n"
            "assert 'rgbid.refine' not in sys.modules\n"
            "assert inspect.signature(TS.fuse).parameters['refine'].default is None\n"
            "assert inspect.signature(TS.Volume.extract).parameters['refine'].default is None\n"
            "def fuse(**kw):\n"
            "    try:\n"
            "        TS.fuse(None, [], (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), **kw)\n"
            "    except ValueError as e:\n"
            "        assert 'no keyframes' in str(e), e\n"
            "fuse(); fuse(refine=None, fill_holes=3, smooth=None); assert 'rgbid.refine' not in sys.modules\n"
            "fuse(refine=0.05); assert 'rgbid.refine' in sys.modules\n") % (ROOT, os.path.join(ROOT, "rgbid-slam_amd"))
    subprocess.check_call([sys.executable, "-c", code])


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_refine.c"
    src.write_text('#include "rgbid_refine.h"\n'
                   "int use(rgbid_refine* h, rgbid_ctx* ctx, const float* v, const uint8_t* c, const float* n, const uint32_t* tris, const uint8_t* s,\n"
                   "        float* vo, uint8_t* co, float* no, uint32_t* to, uint8_t* so) {\n"
                   "  unsigned long long counts[9]; float ms[2];\n"
                   "  return rgbid_refine_create(&h, ctx, RGBID_REFINE_MAX_VERTICES, RGBID_REFINE_MAX_TRIANGLES)\n"
                   "       + rgbid_refine_plan(h, 10, 5, tris, v, s, 0.05, counts)\n"
                   "       + rgbid_refine_emit(h, v, c, n, tris, s, vo, co, no, to, so, 10 + counts[2], 5 + counts[8])\n"
                   "       + rgbid_refine_timing(h, 1, ms) + rgbid_refine_destroy(h); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_refine.h")).read()
    num = lambda name: int(re.search(r"RGBID_REFINE_%s\s+(\d+)ull" % name, txt).group(1))
    assert num("MAX_VERTICES") == RF.MAX_VERTICES == RM.MAX_VERTICES == 1 << 31
    assert num("MAX_TRIANGLES") == RF.MAX_TRIANGLES == RM.MAX_TRIANGLES == 1 << 29
    assert "116 bytes per triangle of capacity" in " ".join(txt.split()) and "0 bytes per vertex of capacity" in " ".join(txt.split())


def test_library_exports_refine_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_refine.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_refine_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(RF.EXPORTS) and len(declared) == 5, set(declared) ^ set(RF.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    for name, types in RF.SIGNATURES.items():
        getattr(L, name).argtypes = list(types)
    h = c.c_void_p()
    assert L.rgbid_refine_create(c.byref(h), None, 10, 10) == -1 and not h.value and L.rgbid_refine_create(None, None, 10, 10) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        assert L.rgbid_refine_create(c.byref(h), fake, v, t) == -1 and not h.value
    assert L.rgbid_refine_plan(None, 0, 0, None, None, None, 0.1, None) == -1
    assert L.rgbid_refine_emit(None, None, None, None, None, None, None, None, None, None, None, 0, 0) == -1
    assert L.rgbid_refine_timing(None, 0, None) == -1 and L.rgbid_refine_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-refine", "0.05"], "--mesh-refine needs --mesh"),
                      (mesh_opt + ["--mesh-refine-rounds", "2", "--mesh-refine-caps"], "need --mesh-refine"),
                      (mesh_opt + ["--mesh-refine", "0.05", "--mesh-refine-caps"], "--mesh-refine-caps needs --mesh-fill-holes"),
                      (mesh_opt + ["--mesh-refine", "-0.05"], "max_edge must be a finite length"), (mesh_opt + ["--mesh-refine", "nan"], "max_edge"),
                      (mesh_opt + ["--mesh-refine", "0.05", "--mesh-refine-rounds", "17"], "rounds must lie in")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()


def test_refined_mesh_through_the_ply_writer(tmp_path):
    v, c, t, n, s, fig = refined("cube_0.11")
    path = tmp_path / "refined.ply"
    TS.write_mesh_ply(str(path), v, c, t, n)
    pv, pc, pt, pn = TS.read_mesh_ply(path.read_bytes())
    assert pv.tobytes() == v.tobytes() and pc.tobytes() == c.tobytes() and pt.tobytes() == t.tobytes() and pn.tobytes() == n.tobytes()
