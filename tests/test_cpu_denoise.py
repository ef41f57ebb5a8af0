"""CPU checks of the denoising stage (include/rgbid_denoise.h, rgbid.denoise): the vectorised numpy restatement the GPU tests compare the
kernels against (tests/denoise_mirror.py) against its scalar loops on every mesh below, and by hand what each mesh is about: the noisy unit
cube with the figures of DESIGN.md section 32 (and Taubin's on the same mesh), the clean cube as a fixed point, the cube with one face
removed, the degenerate triangles, duplicates, non-finite vertices and their payloads, a lone triangle, faces at 90 degrees, a crease, the
order of the vertex pass's sum; empty inputs; the Python argument checks one by one; the header as C99; the library's exports; the command
line's option errors; that nothing is imported without the option."""
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
from rgbid import denoise as DN
from tests import denoise_mirror as DM
from tests import smooth_mirror as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
SNAN_BITS = 0x7F800001                                   # a signalling NaN
SNAN = np.array([SNAN_BITS], U32).view(F)[0]
CELLS = 12
RUNS = ((5, 10, 0.4), (10, 15, 0.5), (20, 20, 0.6), (5, 10, 0.0))      # normal iterations, vertex iterations, T: the rows of section 32


def mesh(vertices, triangles, **more):
    return dict(vertices=np.array(vertices, F).reshape(-1, 3), triangles=np.array(triangles, U32).reshape(-1, 3), **more)


# ---- the cube ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cube():
    """the unit cube with CELLS cells per edge, shared vertices on the edges, numbered as the faces first name them; every cell is cut along
    the same diagonal -> dict(vertices, triangles, face [n_t] = (axis, side) of every triangle, edge bool [n_v]: on an edge of the cube)"""
    n, index, pts, tris, face = CELLS, {}, [], [], []

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
                    outward = (side == n) == (axis != 1)          # e_u x e_v is +e_axis for the axes 0 and 2, -e_axis for 1
                    for t in ((p00, p10, p11), (p00, p11, p01)):
                        tris.append(t if outward else t[::-1])
                        face.append((axis, side))
    lattice = np.array(pts)
    edge = ((lattice == 0) | (lattice == n)).sum(1) >= 2
    return mesh(lattice.astype(np.float64) / n, tris, face=face, edge=edge)


@functools.lru_cache(maxsize=None)
def noisy_vertices():
    """the cube's vertices plus default_rng(7).normal(0, 0.2 / CELLS) on every coordinate, as committed under tests/golden: numpy does not
    promise the stream of `normal` across versions"""
    path = os.path.join(ROOT, "tests", "golden", "denoise_cube_noisy.f32")
    return np.fromfile(path, F).reshape(-1, 3)


def open_cube():
    c = cube()
    keep = np.array([f != (2, CELLS) for f in c["face"]])
    return mesh(noisy_vertices(), c["triangles"][keep], face=[f for f in c["face"] if f != (2, CELLS)], edge=c["edge"])


def distance_to_cube(p):
    q = np.abs(p.astype(np.float64) - 0.5) - 0.5
    d = np.linalg.norm(np.maximum(q, 0), axis=1)
    inside = (q < 0).all(1)
    d[inside] = -q[inside].max(1)
    return d


def rms(p, mask=None):
    d = distance_to_cube(p)
    return float(np.sqrt((d[mask if mask is not None else slice(None)] ** 2).mean()))


def normal_error(p, m):
    """the mean angle in degrees between a face's normal and its true face's, and the share in per cent of the faces above 10 degrees"""
    p, t = p.astype(np.float64), m["triangles"].astype(np.int64)
    n = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    n /= np.linalg.norm(n, axis=1)[:, None]
    true = np.zeros_like(n)
    for i, (axis, side) in enumerate(m["face"]):
        true[i, axis] = 1 if side else -1
    angle = np.degrees(np.arccos(np.clip((n * true).sum(1), -1, 1)))
    return float(angle.mean()), float((angle > 10).mean() * 100)


def volume(p, t):
    p, t = p.astype(np.float64), t.astype(np.int64)
    return float(np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6)


# ---- the hand-built mesh ---------------------------------------------------------------------------------------------------------------
C45, S45, C75, S75 = (math_fn(np.radians(a)) for a in (45.0, 75.0) for math_fn in (np.cos, np.sin))


def hand_mesh():
    v = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0),                                  # 0 - 3: a square, its first triangle given twice
         (5, 5, 5),                                                                   # 4: no triangle names it
         (0, 0, 2), (1, 0, 2),                                                        # 5 - 6: (a, a, b), (a, b, a), (a, a, a)
         (NAN, 0, 4), (0, INF, 4), (0, 0, 4), (1, 0, 4), (SNAN, 1, 4),                # 7 - 11: triangles that are not measurable
         (0, 0, 6), (1, 0, 6), (0, 1, 6),                                             # 12 - 14: a lone triangle
         (0, 0, 10), (1, 0, 10), (0, 1, 10), (0, 0, 11),                              # 15 - 18: +z and +y, exactly 90 degrees
         (0, 0, 20), (1, 0, 20), (0, 1, 20), (0.5, -C45, 20 - S45), (-C75, 0.5, 20 - S75)]   # 19 - 23: B flat, A at 45, C at 75 degrees to B
    t = [(0, 1, 2), (0, 1, 2), (1, 3, 2), (5, 5, 6), (5, 6, 5), (5, 5, 5), (7, 9, 10), (8, 10, 9), (11, 9, 10), (12, 13, 14), (15, 16, 17),
         (16, 15, 18), (19, 20, 21), (20, 19, 22), (19, 21, 23)]
    return mesh(v, t)


@functools.lru_cache(maxsize=None)
def all_cases():
    c = cube()
    rng = np.random.default_rng(7)
    fan = np.stack([np.full(1024, 2048), 2 * np.arange(1024), 2 * np.arange(1024) + 1], 1)
    cases = {"hand": hand_mesh(), "no_triangles": mesh([(0.1, 0.2, 0.3), (4, 5, 6), (NAN, 1, 2)], []), "no_vertices": mesh([], []),
             "cube": mesh(c["vertices"], c["triangles"]), "noisy_cube": mesh(noisy_vertices(), c["triangles"]),
             "open_cube": mesh(noisy_vertices(), open_cube()["triangles"]),
             "fan": mesh(rng.uniform(-1, 1, (2049, 3)), fan),                          # a hub row of 1 024: every face merges it
             "hub_repeats": mesh(rng.uniform(-1, 1, (40, 3)), [(0, k, 0) for k in range(1, 20)] + [(0, k, k + 1) for k in range(20, 39)]),
             "random": mesh(rng.random((300, 3)), rng.integers(0, 300, (2000, 3)))}
    cases["random"]["vertices"][5::97, 1] = NAN              # non-finite vertices among the random ones
    cases["random"]["vertices"][11::101, 2] = INF
    return cases


@functools.lru_cache(maxsize=None)
def table_of(name):
    """the vectorised mirror's face table of a case, computed once and shared with the GPU tests"""
    m = all_cases()[name]
    return DM.face_table(m["triangles"], len(m["vertices"]))


@functools.lru_cache(maxsize=None)
def normals_of(name, iterations, threshold=0.4):
    return DM.normals(all_cases()[name]["vertices"], table_of(name), iterations, threshold)


@functools.lru_cache(maxsize=None)
def denoised(name, normal_iterations, vertex_iterations, threshold=0.4):
    """the positions after both stages"""
    return DM.vertices(all_cases()[name]["vertices"], normals_of(name, normal_iterations, threshold), table_of(name), vertex_iterations)


def words(a):
    return np.ascontiguousarray(a, F).view(U32)


# ---- mirror against loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_mirror_equals_the_loops(name):
    m = all_cases()[name]
    a, b = table_of(name), DM.face_table_loop(m["triangles"], len(m["vertices"]))
    assert DM.same_table(a, b) == [], (name, DM.same_table(a, b), a["counts"], b["counts"])
    assert len(a["faces"]) == 3 * len(m["triangles"]) and int(a["offsets"][-1]) == len(a["faces"])
    assert DM.raw_normals(m["vertices"], a).tobytes() == DM.raw_normals_loop(m["vertices"], b).tobytes()
    for T in (0.0, 0.4, 0.9):
        got = (denoised(name, 2, 2, T), normals_of(name, 2, T))
        exp = DM.denoise_loop(m["vertices"], None, 2, 2, T, tab=b)
        assert got[0].dtype == F and got[1].dtype == F
        assert got[1].tobytes() == exp[1].tobytes() and got[0].tobytes() == exp[0].tobytes(), (name, T)


def test_committed_noise_is_the_generators():
    """the committed vertices are the cube's plus the generator's noise, wherever numpy still draws the stream of the day they were made"""
    c = cube()
    assert len(c["vertices"]) == 866 and len(c["triangles"]) == 1728 and noisy_vertices().shape == (866, 3)
    again = (c["vertices"].astype(np.float64) + np.random.default_rng(7).normal(0, 0.2 / CELLS, (866, 3))).astype(F)
    assert np.abs(noisy_vertices() - c["vertices"]).max() < 0.08
    if again.tobytes() != noisy_vertices().tobytes():
        print("numpy draws another stream than the one committed")


# ---- the cube's figures ----------------------------------------------------------------------------------------------------------------------
def test_cube_topology():
    tab = table_of("cube")
    rows = np.diff(tab["offsets"].astype(np.int64))
    t, _ = DM.neighbourhoods(tab)
    members = np.bincount(t)
    assert (rows.min(), rows.max()) == (4, 6) and (members.min(), members.max()) == (11, 13) and round(float(members.mean()), 2) == 12.97
    assert tab["counts"] == dict(empty_rows=0, longest_row=6, repeating_triangles=0, work=int(rows[tab["triangles"]].sum()))
    assert cube()["edge"].sum() == 8 + 12 * (CELLS - 1)


def test_noisy_cube_figures():
    """section 32's table, to the digits printed"""
    c, noisy = cube(), noisy_vertices()
    figures = lambda p, digits=1: (round(rms(p), 5), round(rms(p, c["edge"]), 5), round(normal_error(p, c)[0], 2), round(normal_error(p, c)[1], digits))
    assert figures(noisy, 0) == (0.01697, 0.01894, 20.28, 79) and round(volume(noisy, c["triangles"]), 5) == 1.00452
    exp = {(5, 10, 0.4): (0.00612, 0.01003, 3.19, 2.0), (10, 15, 0.5): (0.00513, 0.00867, 2.35, 1.0), (20, 20, 0.6): (0.00448, 0.0075, 2.32, 1.3),
           (5, 10, 0.0): (0.00667, 0.01088, 3.99, 6.4)}
    for run in RUNS:
        out = denoised("noisy_cube", *run)
        print(run, figures(out), volume(out, c["triangles"]))
        assert figures(out) == exp[run], (run, figures(out))
    assert round(volume(denoised("noisy_cube", 5, 10, 0.4), c["triangles"]), 5) == 1.00466
    taubin = SM.smooth(noisy, c["triangles"], 10, 0.5, -0.53)
    assert figures(taubin, 0) == (0.01001, 0.01106, 9.8, 33) and round(volume(taubin, c["triangles"]), 5) == 1.01003, figures(taubin)


def test_clean_cube_is_a_fixed_point():
    c = cube()
    for run in RUNS:
        assert denoised("cube", *run).tobytes() == c["vertices"].tobytes()
    n = normals_of("cube", 5)
    assert np.array_equal(n, DM.raw_normals(c["vertices"], table_of("cube"))) and set(np.abs(n).sum(1).tolist()) == {1.0}      # a -0 becomes 0
    taubin = SM.smooth(c["vertices"], c["triangles"], 10, 0.5, -0.53)      # ... and Taubin's filter rounds its edges
    assert round(rms(taubin), 5) == 0.00769 and (round(normal_error(taubin, c)[0], 2), round(normal_error(taubin, c)[1])) == (7.4, 31), normal_error(taubin, c)


def test_open_cube_needs_no_pinned_rim():
    m, tab = open_cube(), table_of("open_cube")
    noisy, out = noisy_vertices(), denoised("open_cube", 5, 10, 0.4)
    used = np.zeros(len(noisy), bool)
    used[m["triangles"].reshape(-1)] = True
    inc = SM.adjacency(m["triangles"], len(noisy))
    rim = inc["boundary"] == 1
    assert len(m["triangles"]) == 1440 and used.sum() == 745 and rim.sum() == 48 and tab["counts"]["empty_rows"] == 121
    assert (round(rms(noisy, used), 5), round(rms(out, used), 5)) == (0.01698, 0.00685)
    assert (round(rms(noisy, rim), 5), round(rms(out, rim), 5)) == (0.01755, 0.01302)
    assert round(float(np.abs(out.astype(np.float64) - noisy).max()), 4) == 0.0474
    assert out[~used].tobytes() == noisy[~used].tobytes()


def test_order_of_the_normal_sum_does_not_survive_the_rounding():
    """the honest limit: on the noisy cube the members of F(t) added in descending order give the bytes of the ascending sum on every face
    after 1 and after 5 passes, so no test pins that order"""
    tab = table_of("noisy_cube")
    t, j = DM.neighbourhoods(tab)
    back = dict(tab, pairs=(t[::-1].copy(), j[::-1].copy()))      # np.add.at now meets every F(t) in descending j
    n = m = DM.raw_normals(noisy_vertices(), tab)
    for k in range(5):
        n, m = DM.normal_pass(n, tab, 0.4), DM.normal_pass(m, back, 0.4)
        assert k not in (0, 4) or n.tobytes() == m.tobytes()


# ---- the hand-built mesh -----------------------------------------------------------------------------------------------------------------
def test_hand_built_table_and_raw_normals():
    tab = table_of("hand")
    row = lambda v: tab["faces"][tab["offsets"][v]:tab["offsets"][v + 1]].tolist()
    assert row(0) == [0, 1] and row(1) == [0, 1, 2] and row(2) == [0, 1, 2] and row(3) == [2] and row(4) == []
    assert row(5) == [3, 3, 4, 4, 5, 5, 5] and row(6) == [3, 4]          # a triangle that names a vertex twice stands twice, adjacent
    assert row(9) == [6, 7, 8] and row(12) == [9] and row(19) == [12, 13, 14]
    assert tab["counts"] == dict(empty_rows=1, longest_row=7, repeating_triangles=3, work=sum(len(row(v)) for t in hand_mesh()["triangles"] for v in t))
    t, j = DM.neighbourhoods(tab)
    members = lambda k: j[t == k].tolist()
    assert members(0) == [0, 1, 2] and members(3) == [3, 4, 5] and members(5) == [3, 4, 5] and members(9) == [9] and members(10) == [10, 11]
    n = normals_of("hand", 0)
    assert n[0].tolist() == [0, 0, 1] and n[1].tolist() == [0, 0, 1] and n[2].tolist() == [0, 0, 1]
    for zero in (3, 4, 5, 6, 7, 8):                            # no area; a NaN, an inf, a signalling NaN at a corner
        assert words(n[zero]).tolist() == [0, 0, 0]
    assert n[9].tolist() == [0, 0, 1] and n[10].tolist() == [0, 0, 1] and n[11].tolist() == [0, 1, 0]


def test_hand_built_normal_pass():
    n0 = normals_of("hand", 0)
    for T in (0.0, 0.4, 0.9):
        n1 = normals_of("hand", 1, T)
        for keep in (3, 4, 5, 6, 7, 8):                          # a zero normal copies its words
            assert words(n1[keep]).tolist() == words(n0[keep]).tolist()
        for keep in (0, 1, 2, 9):                                # flat neighbours, a lone triangle: the normal stays (a -0 becomes 0)
            assert n1[keep].tolist() == n0[keep].tolist() == [0, 0, 1]
    n1 = normals_of("hand", 1, 0.0)
    assert n1[10].tolist() == [0, 0, 1] and n1[11].tolist() == [0, 1, 0]      # the dot product is 0, not above T = 0: neither hears the other
    # B = 12 hears A = 13 (cos 45 > 0.4) and not C = 14 (cos 75 < 0.4); T = 0.2 lets C in
    a, b, c = (n0[k].astype(np.float64) for k in (13, 12, 14))
    dot = lambda x, y: (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
    assert 0.70 < dot(b, a) < 0.71 and 0.25 < dot(b, c) < 0.26 and dot(a, c) < 0.4

    def filtered(T, members):
        s = np.zeros(3)
        for m in members:                                      # ascending triangle number: B, A, C
            w = (dot(b, m) - T) * (dot(b, m) - T)
            s = s + w * m
        return (s / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])).astype(F)

    n1 = normals_of("hand", 1, 0.4)
    assert n1[12].tobytes() == filtered(0.4, (b, a)).tobytes() != filtered(0.4, (b, a, c)).tobytes()
    assert normals_of("hand", 1, 0.2)[12].tobytes() == filtered(0.2, (b, a, c)).tobytes()
    assert np.abs(n1[14] - n0[14]).max() < 1e-7                # C hears itself alone: s = (d - T)^2 n, and n again after the division


def test_hand_built_vertex_pass():
    m, tab = all_cases()["hand"], table_of("hand")
    v = m["vertices"]
    out = DM.vertex_pass(v, normals_of("hand", 0), tab)
    for keep in (0, 1, 2, 3, 4, 7, 8, 11, 12, 13, 14):         # in the plane of their faces; unreferenced; not finite themselves
        assert words(out[keep]).tolist() == words(v[keep]).tolist()
    assert int(words(out[11])[0]) == SNAN_BITS                 # the payload is kept
    for keep in (5, 6, 9, 10):                                 # all their triangles have a zero normal or a corner that is not finite
        assert words(out[keep]).tolist() == words(v[keep]).tolist()
    # vertex 16 lies on the crease of +z and +y: both faces hold it already; vertex 19 is pulled by A, B and C, each once
    assert out[16].tolist() == v[16].tolist()
    n = normals_of("hand", 1, 0.4).astype(np.float64)           # B's normal now leans towards A's
    out = DM.vertex_pass(v, normals_of("hand", 1, 0.4), tab)
    x, s = v[19].astype(np.float64), np.zeros(3)
    for t in (12, 13, 14):
        p = v[m["triangles"][t].astype(np.int64)].astype(np.float64)
        e = ((p[0] + p[1]) + p[2]) / 3.0 - x
        s = s + n[t] * ((n[t][0] * e[0] + n[t][1] * e[1]) + n[t][2] * e[2])
    assert out[19].tobytes() == (x + s / 3.0).astype(F).tobytes() != v[19].tobytes()
    # a repeat counts once: the hub of (0, k, 0) divides by the triangles, not by the entries of its row
    hub, htab = all_cases()["hub_repeats"], table_of("hub_repeats")
    assert htab["counts"]["longest_row"] == 2 * 19 + 19 and htab["counts"]["repeating_triangles"] == 19
    nrm = np.tile(np.array([0, 0, 1], F), (len(hub["triangles"]), 1))
    got = DM.vertex_pass(hub["vertices"], nrm, htab)[0]
    x = hub["vertices"][0].astype(np.float64)
    s = 0.0
    for t in hub["triangles"].astype(np.int64):
        p = hub["vertices"][t].astype(np.float64)
        s = s + (((p[0][2] + p[1][2]) + p[2][2]) / 3.0 - x[2])
    assert got.tolist() == [hub["vertices"][0][0], hub["vertices"][0][1], F(x[2] + s / 38.0)]


def test_vertex_pass_sums_in_ascending_triangle_order():
    """normals 0 0 1 on three triangles around vertex 0 whose centroids lie 1, X and -X above it, X about 1e30: 1 + X - X is 0 in
    ascending order and 1 in descending order"""
    v = mesh([(0, 0, 0), (1, 0, 1.5), (0, 1, 1.5), (1, 0, 1.5e30), (0, 1, 1.5e30), (1, 0, -1.5e30), (0, 1, -1.5e30)], [])["vertices"]
    tri = np.array([(0, 1, 2), (0, 3, 4), (0, 5, 6)], U32)
    nrm = np.tile(np.array([0, 0, 1], F), (3, 1))
    for tab, fn in ((DM.face_table(tri, 7), DM.vertex_pass), (DM.face_table_loop(tri, 7), DM.vertex_pass_loop)):
        out = fn(v, nrm, tab)
        assert out[0].tolist() == [0, 0, 0]
    back = fn(v, nrm[::-1].copy(), DM.face_table_loop(tri[::-1].copy(), 7))      # the same triangles numbered the other way round
    assert back[0].tolist() == [0, 0, F(1 / 3)]
    # normals that are not unit, and one that is not finite: the triangle does not take part
    out = DM.vertex_pass(v, np.array([(0, 0, 2), (NAN, 0, 1), (0, 0, 0)], F), DM.face_table(tri, 7))
    assert out[0].tolist() == [0, 0, 4.0]                      # N (N . e) / m = 2 * 2 * 1 / 1


def centroid_mesh():
    """one triangle whose corners lie at z = X, -X and 1.5, X about 1e30: ((X - X) + 1.5) / 3 is 0.5, (X + (-X + 1.5)) / 3 is 0"""
    return mesh([(0, 0, 1e30), (1, 0, -1e30), (0, 1, 1.5)], [(0, 1, 2)])


def test_centroid_adds_the_corners_in_order():
    m = centroid_mesh()
    nrm = np.array([(0, 0, 1)], F)
    for tab, fn in ((DM.face_table(m["triangles"], 3), DM.vertex_pass), (DM.face_table_loop(m["triangles"], 3), DM.vertex_pass_loop)):
        out = fn(m["vertices"], nrm, tab)
        assert out[2].tolist() == [0, 1, 0.5] and out[0].tolist() == [0, 0, 0] and out[1].tolist() == [1, 0, 0]


# ---- empty and degenerate inputs ---------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    tab = table_of("no_triangles")
    v = all_cases()["no_triangles"]["vertices"]
    assert tab["counts"] == dict(empty_rows=3, longest_row=0, repeating_triangles=0, work=0) and tab["offsets"].tolist() == [0] * 4
    assert denoised("no_triangles", 5, 10).tobytes() == v.tobytes() and normals_of("no_triangles", 5).shape == (0, 3)
    tab = table_of("no_vertices")
    assert tab["counts"] == dict.fromkeys(DM.COUNTS, 0) and tab["offsets"].tolist() == [0] and denoised("no_vertices", 3, 3).shape == (0, 3)
    for name in ("hand", "noisy_cube"):
        m = all_cases()[name]
        assert denoised(name, 3, 0).tobytes() == m["vertices"].tobytes()                    # no vertex iteration returns the bytes
        assert normals_of(name, 0).tobytes() == DM.raw_normals(m["vertices"], table_of(name)).tobytes()
        assert denoised(name, 0, 2).tobytes() == DM.vertices(m["vertices"], normals_of(name, 0), table_of(name), 2).tobytes()
    for bad in ((0, 1, 3), (0, 1, -1)):
        with pytest.raises(ValueError):
            DM.face_table([bad], 3)
        with pytest.raises(ValueError):
            DM.face_table_loop([bad], 3)
    for n, T in ((257, 0.4), (-1, 0.4), (1, 1.0), (1, -0.1), (1, NAN)):
        with pytest.raises(ValueError):
            DM.normals(v, table_of("no_triangles"), n, T)


# ---- the Python checkers, one by one ------------------------------------------------------------------------------------------------------
def test_checkers():
    assert DN.capacity_arg(1, 1) == (1, 1) and DN.capacity_arg(1 << 31, np.int64(1 << 29)) == (1 << 31, 1 << 29)
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 1), (1, (1 << 29) + 1), (-1, 1), (1.0, 1), (1, "1"), (None, 1), (True, 1)):
        with pytest.raises(ValueError):
            DN.capacity_arg(v, t)
    assert DN.iterations_arg(0) == 0 and DN.iterations_arg(np.int32(256)) == 256
    for n in (-1, 257, 1.0, "3", None, True):
        with pytest.raises(ValueError):
            DN.iterations_arg(n)
    assert DN.threshold_arg(0) == 0.0 and DN.threshold_arg(np.float32(0.5)) == 0.5 and DN.threshold_arg(0.999) == 0.999
    for T in (-0.1, 1, 1.5, NAN, INF, "0.4", None, True):
        with pytest.raises(ValueError):
            DN.threshold_arg(T)
    assert DN.denoise_arg(None) is None and DN.denoise_arg(3) == dict(normal_iterations=3, vertex_iterations=10, threshold=0.4)
    assert DN.denoise_arg(dict(normal_iterations=2, vertex_iterations=0, threshold=0)) == dict(normal_iterations=2, vertex_iterations=0, threshold=0.0)
    for bad in (-1, 257, 1.5, "3", dict(threshold=0.5), dict(normal_iterations=3, iterations=1), dict(normal_iterations=3, threshold=1),
                dict(normal_iterations=3, vertex_iterations=257), dict(normal_iterations=3, vertex_iterations=1.0)):
        with pytest.raises(ValueError):
            DN.denoise_arg(bad)


def test_mesh_checker_needs_cuda_tensors():
    import torch
    ht = torch.zeros((4, 3), dtype=torch.int32)
    for t, n in ((ht, 5), (ht.numpy(), 5), (None, 5)):
        with pytest.raises(ValueError):
            DN.mesh_arg(t, n)


def test_checks_come_before_the_library():
    from rgbid import tsdf as TS
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 4), (4, (1 << 29) + 1)):
        with pytest.raises(ValueError):
            DN.Denoiser(None, v, t)

    class Ctx:
        device = 0
    dn = DN.Denoiser.__new__(DN.Denoiser)
    dn.ctx, dn.max_vertices, dn.max_triangles, dn._triangles, dn.counts, dn.n_vertices, dn.n_triangles = Ctx(), 10, 10, None, None, 0, 0
    with pytest.raises(ValueError):
        dn.plan(np.zeros((1, 3), np.int32), 3)
    for call in (lambda: dn.normals(None), lambda: dn.normals_into(None, None), lambda: dn.vertices(None, None), lambda: dn.vertices_into(None, None, None),
                 lambda: dn.faces(), lambda: dn.run(None)):
        with pytest.raises(ValueError):
            call()                                                  # nothing is planned
    for kw in (dict(normal_iterations=-1), dict(vertex_iterations=257), dict(threshold=1.0)):
        with pytest.raises(ValueError):
            dn.run(None, **kw)
        with pytest.raises(ValueError):
            DN.denoise_mesh(None, None, None, **kw)
    with pytest.raises(ValueError):
        DN.denoise_mesh(None, None, None)                           # no tensors
    dn._h = None
    kf = [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)]
    for s in (-1, 1.5, dict(threshold=0.5), dict(normal_iterations=1, threshold=2)):
        with pytest.raises(ValueError):
            TS.fuse(None, kf, (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), denoise=s)
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels = Ctx(), 2, 1000
    for s in (-1, dict(normal_iterations=1, vertex_iterations=-3)):
        with pytest.raises(ValueError):
            vol.extract(1, denoise=s)
    vol._h = None


def test_nothing_is_imported_without_the_option():
    code = ("import sys; sys.path[:0] = [%r, %r]; from rgbid import tsdf as TS; import inspect; "
            "assert inspect.signature(TS.Volume.extract).parameters['denoise'].default is None; "
            "assert inspect.signature(TS.fuse).parameters['denoise'].default is None; "
            "assert 'rgbid.denoise' not in sys.modules; from rgbid import denoise; assert denoise.denoise_arg(None) is None") % (
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
    src = tmp_path / "use_denoise.c"
    src.write_text('#include "rgbid_denoise.h"\n'
                   "int use(rgbid_denoise* h, rgbid_ctx* ctx, const float* v, const uint32_t* tris, float* vo, float* no, uint32_t* off, uint32_t* fc) {\n"
                   "  unsigned long long counts[4]; float ms[3];\n"
                   "  return rgbid_denoise_create(&h, ctx, RGBID_DENOISE_MAX_VERTICES, RGBID_DENOISE_MAX_TRIANGLES)\n"
                   "       + rgbid_denoise_plan(h, 10, 5, tris, counts) + rgbid_denoise_faces(h, off, fc)\n"
                   "       + rgbid_denoise_normals(h, v, no, RGBID_DENOISE_MAX_ITERATIONS, 0.4)\n"
                   "       + rgbid_denoise_vertices(h, v, no, vo, 10u) + rgbid_denoise_timing(h, 1, ms) + rgbid_denoise_destroy(h); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_denoise.h")).read()
    assert int(re.search(r"RGBID_DENOISE_MAX_VERTICES\s+(\d+)ull", txt).group(1)) == DN.MAX_VERTICES == 1 << 31
    assert int(re.search(r"RGBID_DENOISE_MAX_TRIANGLES\s+(\d+)ull", txt).group(1)) == DN.MAX_TRIANGLES == 1 << 29
    assert int(re.search(r"RGBID_DENOISE_MAX_ITERATIONS\s+(\d+)u", txt).group(1)) == DN.MAX_ITERATIONS == DM.MAX_ITERATIONS == 256


def test_library_exports_denoise_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_denoise.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_denoise_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(DN.EXPORTS) and len(declared) == 7, set(declared) ^ set(DN.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    L.rgbid_denoise_create.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_ulonglong]
    L.rgbid_denoise_plan.argtypes = [c.c_void_p, c.c_ulonglong, c.c_ulonglong, c.c_void_p, c.c_void_p]
    L.rgbid_denoise_faces.argtypes = [c.c_void_p] * 3
    L.rgbid_denoise_normals.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint, c.c_double]
    L.rgbid_denoise_vertices.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint]
    L.rgbid_denoise_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_denoise_destroy.argtypes = [c.c_void_p]
    h = c.c_void_p()
    assert L.rgbid_denoise_create(c.byref(h), None, 10, 10) == -1 and not h.value and L.rgbid_denoise_create(None, None, 10, 10) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        assert L.rgbid_denoise_create(c.byref(h), fake, v, t) == -1 and not h.value
    assert L.rgbid_denoise_plan(None, 0, 0, None, None) == -1 and L.rgbid_denoise_faces(None, None, None) == -1
    assert L.rgbid_denoise_normals(None, None, None, 1, 0.4) == -1 and L.rgbid_denoise_vertices(None, None, None, None, 1) == -1
    assert L.rgbid_denoise_timing(None, 0, None) == -1 and L.rgbid_denoise_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-denoise", "5"], "--mesh-denoise needs --mesh"),
                      (mesh_opt + ["--mesh-denoise-vertex-iterations", "5"], "need --mesh-denoise"),
                      (mesh_opt + ["--mesh-denoise-threshold", "0.5"], "need --mesh-denoise"),
                      (mesh_opt + ["--mesh-denoise", "257"], "normal_iterations must lie in"), (mesh_opt + ["--mesh-denoise", "x"], "invalid int value"),
                      (mesh_opt + ["--mesh-denoise", "3", "--mesh-denoise-vertex-iterations", "-1"], "vertex_iterations must lie in"),
                      (mesh_opt + ["--mesh-denoise", "3", "--mesh-denoise-threshold", "1"], "threshold must be"),
                      (mesh_opt + ["--mesh-denoise", "3", "--mesh-denoise-threshold", "nan"], "threshold must be")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()
