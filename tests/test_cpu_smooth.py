"""CPU checks of the smoothing stage (include/rgbid_smooth.h, rgbid.smooth): the vectorised numpy restatement the GPU tests compare the
kernels against (tests/smooth_mirror.py) against its scalar loops on every mesh below, and by hand what each mesh is about: the three
degenerate triangles, duplicates, a non-manifold edge, rims, non-finite vertices and their payloads, a vertex that overflows, the order of
the sums; empty inputs; section 19's sphere with the figures of the issue (no shrinkage under Taubin's factors, shrinkage without mu, noise
removed, area-weighted normals); the sphere cut open with its boundary pinned and not; the Python argument checks one by one; the header as
C99; the library's exports; the command line's option errors; a smoothed mesh through the PLY writer."""
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
from rgbid import smooth as SO
from rgbid import tsdf as TS
from tests import smooth_mirror as SM
from tests import tsdf_mirror as TM
from tests.test_cpu_mesh import hard_meshes, tsdf_meshes
from tests.test_cpu_simplify import signed_volume
from tests.test_cpu_tsdf import SPHERE, sphere_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
SNAN_BITS = 0x7F800001                                   # a signalling NaN
SNAN = np.array([SNAN_BITS], U32).view(F)[0]


def mesh(vertices, triangles):
    return dict(vertices=np.array(vertices, F).reshape(-1, 3), triangles=np.array(triangles, U32).reshape(-1, 3))


# ---- the meshes: name -> dict(vertices float32 [n_v, 3], triangles uint32 [n_t, 3]) --------------------------------------------------------
def hand_mesh():
    v = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0),                                  # 0 - 3: two triangles, each given twice
         (2, 0, 0), (3, 0, 0), (2, 1, 0), (2, -1, 0), (2, 0, 1),                      # 4 - 8: the edge 4 5 in three triangles, rims
         (5, 5, 5),                                                                   # 9: no triangle names it
         (0, 0, 2), (1, 0, 2), (0, 0, 3), (1, 0, 3), (0, 0, 4),                       # 10 - 14: (a, a, b), (a, b, a), (a, a, a)
         (0, 0, 5), (NAN, 0, 0), (0, INF, 0),                                         # 15 - 17: all neighbours of 15 are not finite
         (SNAN, 0.5, 0.5), (0, 0, 6), (1, 0, 6), (0, 1, 6),                           # 18 - 21: a tetrahedron whose apex is a signalling NaN
         (3e38, 0, 0), (-3e38, 0, 0), (-3e38, 1, 0),                                  # 22 - 24: a pass with mu = -1 takes 22 to inf
         (2, 0, 0), (1e30, 0, 0), (1, 0, 0), (-1e30, 0, 0),                           # 25 - 28: the cancellation star, 1e30 + 1 - 1e30 = 0
         (2, 0, 0), (1, 0, 0), (1e30, 0, 0), (-1e30, 0, 0)]                           # 29 - 32: 1 + 1e30 - 1e30 = 0, descending it is 1
    t = [(0, 1, 2), (0, 1, 2), (1, 0, 3), (1, 0, 3), (4, 5, 6), (4, 5, 7), (4, 5, 8), (10, 10, 11), (12, 13, 12), (14, 14, 14), (15, 16, 17),
         (18, 19, 20), (18, 20, 21), (18, 21, 19), (19, 21, 20), (22, 23, 24), (25, 26, 27), (25, 27, 28), (29, 30, 31), (29, 31, 32)]
    return mesh(v, t)


def open_sphere():
    vol = sphere_volume()
    vol.W[:, :, :12] = 2
    v, _, t = TM.extract(vol, 2)
    return mesh(v, t)


def random_positions(n_v, seed):
    return np.random.default_rng(900 + seed).uniform(-1, 1, (n_v, 3)).astype(F)


@functools.lru_cache(maxsize=None)
def all_cases():
    ts = tsdf_meshes()
    strip, fan = hard_meshes()["strip"], hard_meshes()["fan"]
    rng = np.random.default_rng(7)
    cases = {"hand": hand_mesh(), "no_triangles": mesh([(0.1, 0.2, 0.3), (4, 5, 6), (NAN, 1, 2)], []), "no_vertices": mesh([], []),
             "sphere": mesh(ts["sphere"][0], ts["sphere"][2]), "open_sphere": open_sphere(),
             "two_spheres": mesh(ts["two_spheres"][0], ts["two_spheres"][2]), "noise": mesh(ts["noise"][0], ts["noise"][2]),
             "strip": mesh(random_positions(strip[1], 1), strip[0]), "fan": mesh(random_positions(fan[1], 2), fan[0]),
             "random": mesh(rng.random((3000, 3)), rng.integers(0, 3000, (20000, 3)))}
    cases["random"]["vertices"][5::97, 1] = NAN              # non-finite vertices among the random ones
    cases["random"]["vertices"][11::201, 2] = INF
    return cases


@functools.lru_cache(maxsize=None)
def adjacency_of(name):
    """the vectorised mirror's adjacency of a case, computed once and shared with the GPU tests"""
    m = all_cases()[name]
    return SM.adjacency(m["triangles"], len(m["vertices"]))


@functools.lru_cache(maxsize=None)
def smoothed(name, iterations, lam=0.5, mu=-0.53, pin=False):
    return SM.smooth(all_cases()[name]["vertices"], None, iterations, lam, mu, pin, adj=adjacency_of(name))


@functools.lru_cache(maxsize=None)
def normals_of(name):
    return SM.normals(all_cases()[name]["vertices"], adjacency_of(name))


def words(a):
    return np.ascontiguousarray(a, F).view(U32)


# ---- mirror against loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_mirror_equals_the_loops(name):
    m = all_cases()[name]
    a, b = adjacency_of(name), SM.adjacency_loop(m["triangles"], len(m["vertices"]))
    assert SM.same_adjacency(a, b) == [], (name, SM.same_adjacency(a, b), a["counts"], b["counts"])
    c = a["counts"]
    assert c["pairs"] == 2 * c["edges"] == len(a["neighbours"]) and len(a["corners"]) == 3 * len(m["triangles"])
    assert int(a["incidences"].sum()) + c["dropped"] == 6 * len(m["triangles"])
    for mu in (-0.53, 0.0):
        for pin in (False, True):
            got, exp = smoothed(name, 2, 0.5, mu, pin), SM.smooth_loop(m["vertices"], None, 2, 0.5, mu, pin, adj=b)
            assert got.dtype == F and got.tobytes() == exp.tobytes(), (name, mu, pin)
    assert normals_of(name).tobytes() == SM.normals_loop(m["vertices"], b).tobytes()
    assert SM.normals(smoothed(name, 2), a).tobytes() == SM.normals_loop(smoothed(name, 2), b).tobytes()


def test_sums_are_sequential_in_neighbour_order():
    """a row of 100 000 neighbours whose values lose bits in any other order of adding: np.add.at against the scalar loop"""
    n = 100000
    rng = np.random.default_rng(3)
    v = (rng.random((n + 2, 3)) * np.array([1.0, 1e-3, 1e3])).astype(F)
    tri = np.stack([np.full(n, n + 1), np.arange(n), np.arange(1, n + 1)], 1)        # a fan around the last vertex
    a, b = SM.adjacency(tri, n + 2), SM.adjacency_loop(tri, n + 2)
    assert SM.same_adjacency(a, b) == [] and a["counts"]["max_degree"] == n + 1
    got, exp = SM.smooth_pass(v, a, 0.5), SM.smooth_pass_loop(v, b, 0.5)
    assert got.tobytes() == exp.tobytes()
    fwd, back = [0.0] * 3, [0.0] * 3
    for row in v[:n + 1]:
        for k in range(3):
            fwd[k] += float(row[k])
    for row in v[n::-1]:
        for k in range(3):
            back[k] += float(row[k])
    assert fwd != back                                        # the order matters on this input ...
    hub = [float(x) for x in v[n + 1]]
    assert got[n + 1].tolist() == [F(hub[k] + 0.5 * (fwd[k] / float(n + 1) - hub[k])) for k in range(3)]      # ... and the mirror's is ascending


# ---- the hand-built mesh -----------------------------------------------------------------------------------------------------------------
def test_hand_built_adjacency():
    a = adjacency_of("hand")
    assert a["counts"] == dict(pairs=72, edges=36, boundary_pairs=40, boundary_vertices=19, isolated=2, max_degree=4, dropped=10, non_manifold=4)
    row = lambda v: (a["neighbours"][a["offsets"][v]:a["offsets"][v + 1]].tolist(), a["incidences"][a["offsets"][v]:a["offsets"][v + 1]].tolist())
    assert row(0) == ([1, 2, 3], [4, 2, 2]) and row(1) == ([0, 2, 3], [4, 2, 2])        # every triangle twice: the shared edge four times
    assert row(4) == ([5, 6, 7, 8], [3, 1, 1, 1]) and row(6) == ([4, 5], [1, 1])        # an edge in three triangles, rims
    assert row(9) == ([], []) and row(14) == ([], [])                                   # unreferenced; (a, a, a) names it and gives no pair
    assert row(10) == ([11], [2]) and row(11) == ([10], [2])                            # (a, a, b)
    assert row(12) == ([13], [2]) and row(13) == ([12], [2])                            # (a, b, a): two corners join the two
    assert row(25) == ([26, 27, 28], [1, 2, 1])
    assert a["boundary"].tolist() == [0] * 4 + [1] * 5 + [0] * 6 + [1] * 3 + [0] * 4 + [1] * 11
    corners = lambda v: a["corners"][a["corner_offsets"][v]:a["corner_offsets"][v + 1]].tolist()
    assert corners(0) == [0, 3, 7, 10] and corners(14) == [27, 28, 29] and corners(12) == [24, 26] and corners(9) == []


def test_hand_built_pass():
    m, a = all_cases()["hand"], adjacency_of("hand")
    v = m["vertices"]
    one = SM.smooth_pass(v, a, 0.5)
    assert one[0].tolist() == [F(1 / 3), F(1 / 3), 0]         # a duplicate is one neighbour: the mean of 1, 2, 3 and not of 1, 1, 2, 2, 3, 3
    assert one[4].tolist() == [2.125, 0, 0.125]               # the mean of 5, 6, 7, 8 is (2.25, 0, 0.25)
    for keep in (9, 14, 15, 16, 17, 18):                       # no neighbour; none that is finite; not finite itself
        assert words(one[keep]).tolist() == words(v[keep]).tolist()
    assert int(words(one[18])[0]) == SNAN_BITS                 # the payload is kept ...
    assert one[19].tolist() == [0.25, 0.25, 6.0]               # ... and its neighbours skip it: the mean of 20 and 21
    assert one[25].tolist() == [1, 0, 0] and one[29].tolist() == [1, 0, 0]       # both sums are 0 in ascending order, 2 + 0.5 (0 - 2)
    # mu = -1 takes vertex 22 to 3e38 + 6e38 = inf; from then on it stays and its neighbours skip it
    blown = SM.smooth_pass(v, a, -1.0)
    assert blown[22].tolist() == [INF, -0.5, 0.0] and blown[23, 0] == -INF and blown[24, 0] == -INF       # the mean of 23's neighbours is 0 in x
    again = SM.smooth_pass(blown, a, 0.5)
    assert words(again[22:25]).tolist() == words(blown[22:25]).tolist()
    half = blown.copy()
    half[23:25] = v[23:25]                                     # only 22 is not finite: 23 and 24 see each other alone
    assert SM.smooth_pass(half, a, 0.5)[23].tolist() == [float(F(-3e38)), 0.5, 0.0]
    pinned = SM.smooth_pass(v, a, 0.5, pin_boundary=True)
    assert words(pinned[4:9]).tolist() == words(v[4:9]).tolist() and pinned[0].tolist() == one[0].tolist()
    # the run the GPU tests repeat: lambda moves 22 by less than half an ulp, mu = -1 then takes it to inf
    run = SM.smooth(v, None, 2, 1e-9, -1.0, adj=a)
    assert run[22, 0] == INF and int(words(run[18])[0]) == SNAN_BITS


def test_hand_built_normals():
    a = adjacency_of("hand")
    n = normals_of("hand")
    assert n[0].tolist() == [0, 0, 0]                          # (0, 1, 2) twice and (1, 0, 3) twice: +z and -z cancel
    assert n[2].tolist() == [0, 0, 1] and n[3].tolist() == [0, 0, -1]
    assert n[9].tolist() == [0, 0, 0] and n[10].tolist() == [0, 0, 0] and n[14].tolist() == [0, 0, 0]       # no corner; zero-area triangles
    assert n[15].tolist() == [0, 0, 0] and n[18].tolist() == [0, 0, 0]                  # no measurable triangle
    assert n[19].tolist() == [0, 0, -1]                        # only the base (19, 21, 20) is measurable
    assert np.isfinite(n).all() and len(a["corners"]) == 60


# ---- empty and degenerate inputs ---------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    a = adjacency_of("no_triangles")
    assert a["counts"] == dict(pairs=0, edges=0, boundary_pairs=0, boundary_vertices=0, isolated=3, max_degree=0, dropped=0, non_manifold=0)
    assert a["offsets"].tolist() == [0] * 4 and a["corner_offsets"].tolist() == [0] * 4
    v = all_cases()["no_triangles"]["vertices"]
    assert smoothed("no_triangles", 5).tobytes() == v.tobytes() and not normals_of("no_triangles").any()
    a = adjacency_of("no_vertices")
    assert a["counts"] == dict.fromkeys(SM.COUNTS, 0) and a["offsets"].tolist() == [0] and smoothed("no_vertices", 3).shape == (0, 3)
    for name in ("hand", "sphere"):
        assert smoothed(name, 0).tobytes() == all_cases()[name]["vertices"].tobytes()          # iterations = 0 returns the bytes
    # mu = 0 makes half the passes: two iterations are two passes with lambda
    v, a = all_cases()["sphere"]["vertices"], adjacency_of("sphere")
    assert smoothed("sphere", 2, 0.5, 0.0).tobytes() == SM.smooth_pass(SM.smooth_pass(v, a, 0.5), a, 0.5).tobytes()
    assert smoothed("sphere", 1).tobytes() == SM.smooth_pass(SM.smooth_pass(v, a, 0.5), a, -0.53).tobytes()
    for bad in ((0, 1, 3), (0, 1, -1)):
        with pytest.raises(ValueError):
            SM.adjacency([bad], 3)
        with pytest.raises(ValueError):
            SM.adjacency_loop([bad], 3)


# ---- section 19's sphere -------------------------------------------------------------------------------------------------------------------
def test_sphere_topology():
    a = adjacency_of("sphere")
    degree = np.diff(a["offsets"].astype(np.int64))
    assert a["counts"] == dict(pairs=12000, edges=6000, boundary_pairs=0, boundary_vertices=0, isolated=0, max_degree=8, dropped=0, non_manifold=0)
    assert (a["incidences"] == 2).all() and degree.min() == 4 and degree.max() == 8 and not a["boundary"].any()


def test_taubin_keeps_the_volume_and_laplace_shrinks_it():
    m = all_cases()["sphere"]
    before = signed_volume(m["vertices"], m["triangles"])
    taubin, laplace = signed_volume(smoothed("sphere", 10), m["triangles"]), signed_volume(smoothed("sphere", 10, 0.5, 0.0), m["triangles"])
    print("signed volume:", before, "taubin", taubin, "laplace", laplace)      # measured: 0.11152, 0.11195 (+0.4 %), 0.10403 (-6.7 %)
    assert abs(taubin / before - 1.0) < 0.01 and laplace < 0.95 * before


def test_taubin_removes_radial_noise():
    m, a = all_cases()["sphere"], adjacency_of("sphere")
    centre, radius = np.array(SPHERE["centre"]), SPHERE["radius"]
    d = m["vertices"].astype(np.float64) - centre
    r = np.linalg.norm(d, axis=1)
    noisy = (m["vertices"].astype(np.float64) + d / r[:, None] * np.random.default_rng(3).normal(0, 0.005, len(r))[:, None]).astype(F)
    rms = lambda p: float(np.sqrt(((np.linalg.norm(p.astype(np.float64) - centre, axis=1) - radius) ** 2).mean()))
    after = SM.smooth(noisy, None, 10, adj=a)
    print("rms distance to the sphere:", rms(noisy), "->", rms(after))         # measured: 5.02 mm -> 2.06 mm
    assert rms(after) < 0.5 * rms(noisy)


def test_area_weighted_normals_of_the_sphere():
    m, n = all_cases()["sphere"], normals_of("sphere")
    d = m["vertices"].astype(np.float64) - np.array(SPHERE["centre"])
    zero = (n == 0).all(1)
    p = m["vertices"].astype(np.float64)[m["triangles"].astype(np.int64)]
    flat = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0
    assert zero.sum() == 13 and flat.sum() == 147             # coincident vertices: all their triangles have no area
    cos = (n[~zero] * (d / np.linalg.norm(d, axis=1)[:, None])[~zero]).sum(1)
    print("smallest cosine with the radial direction:", cos.min())             # measured: 0.9428
    assert cos.min() > 0.9 and np.allclose(np.linalg.norm(n[~zero].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_open_sphere_pins_its_boundary():
    m, a = all_cases()["open_sphere"], adjacency_of("open_sphere")
    v = m["vertices"]
    assert len(v) == 878 and len(m["triangles"]) == 1676 and a["counts"]["boundary_vertices"] == 78 and a["counts"]["isolated"] == 0
    rim = a["boundary"] == 1
    moved = lambda q: (words(q) != words(v)).any(1)
    pinned, free = smoothed("open_sphere", 1, 0.5, -0.53, True), smoothed("open_sphere", 1)
    assert not moved(pinned)[rim].any() and moved(pinned)[~rim].sum() == 800
    assert moved(free)[rim].sum() == 78 and moved(free)[~rim].sum() == 800


def test_other_meshes():
    assert adjacency_of("fan")["counts"]["max_degree"] == 8192 and adjacency_of("fan")["counts"]["boundary_vertices"] == 8193
    c = adjacency_of("strip")["counts"]
    assert c["isolated"] == 0 and c["boundary_vertices"] == 5002 and c["max_degree"] == 4 and c["edges"] == 2 * 5000 + 1
    c = adjacency_of("random")["counts"]
    assert c["non_manifold"] > 0 and c["dropped"] > 0 and c["isolated"] < 10 and c["max_degree"] > 50
    assert adjacency_of("two_spheres")["counts"]["boundary_vertices"] == 0 and adjacency_of("noise")["counts"]["boundary_vertices"] > 100


# ---- the Python checkers, one by one ------------------------------------------------------------------------------------------------------
def test_checkers():
    assert SO.capacity_arg(1, 1) == (1, 1) and SO.capacity_arg(1 << 31, np.int64(1 << 29)) == (1 << 31, 1 << 29)
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 1), (1, (1 << 29) + 1), (-1, 1), (1.0, 1), (1, "1"), (None, 1), (True, 1)):
        with pytest.raises(ValueError):
            SO.capacity_arg(v, t)
    assert SO.iterations_arg(0) == 0 and SO.iterations_arg(np.int32(4096)) == 4096
    for n in (-1, 4097, 1.0, "3", None, True):
        with pytest.raises(ValueError):
            SO.iterations_arg(n)
    assert SO.factors_arg(0.5, -0.53) == (0.5, -0.53) and SO.factors_arg(1, 0) == (1.0, 0.0) and SO.factors_arg(np.float32(0.25), -2) == (0.25, -2.0)
    for lam, mu in ((0, -0.5), (-0.1, -0.5), (1.01, -0.5), (NAN, -0.5), (INF, -0.5), (0.5, 0.1), (0.5, -2.01), (0.5, NAN), (0.5, -INF), ("0.5", -0.5),
                    (0.5, None), (True, -0.5)):
        with pytest.raises(ValueError):
            SO.factors_arg(lam, mu)
    assert TS.smooth_arg(None) is None and TS.smooth_arg(3) == dict(iterations=3, lam=0.5, mu=-0.53, pin_boundary=False)
    assert TS.smooth_arg(dict(iterations=2, mu=0, pin_boundary=True)) == dict(iterations=2, lam=0.5, mu=0.0, pin_boundary=True)
    for bad in (-1, 4097, 1.5, "3", dict(lam=0.5), dict(iterations=3, cell=1), dict(iterations=3, lam=0), dict(iterations=3, mu=1),
                dict(iterations=3, pin_boundary=1), dict(iterations=3, normals=True)):
        with pytest.raises(ValueError):
            TS.smooth_arg(bad)


def test_mesh_checker_needs_cuda_tensors():
    import torch
    ht = torch.zeros((4, 3), dtype=torch.int32)
    for t, n in ((ht, 5), (ht.numpy(), 5), (None, 5)):
        with pytest.raises(ValueError):
            SO.mesh_arg(t, n)


def test_checks_come_before_the_library():
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 4), (4, (1 << 29) + 1)):
        with pytest.raises(ValueError):
            SO.Smoother(None, v, t)

    class Ctx:
        device = 0
    sm = SO.Smoother.__new__(SO.Smoother)
    sm.ctx, sm.max_vertices, sm.max_triangles, sm._triangles, sm.counts, sm.n_vertices, sm.has_normals = Ctx(), 10, 10, None, None, 0, False
    with pytest.raises(ValueError):
        sm.plan(np.zeros((1, 3), np.int32), 3)
    for call in (lambda: sm.run(None, 1), lambda: sm.run_into(None, None, 1), lambda: sm.adjacency(), lambda: sm.normals(None)):
        with pytest.raises(ValueError):
            call()                                                  # nothing is planned
    for kw in (dict(iterations=-1), dict(iterations=1, lam=0), dict(iterations=1, mu=0.5)):
        with pytest.raises(ValueError):
            sm.run(None, **kw)
        with pytest.raises(ValueError):
            SO.smooth_mesh(None, None, None, **kw)
    with pytest.raises(ValueError):
        SO.smooth_mesh(None, None, None, 1)                         # no tensors
    sm._h = None
    kf = [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)]
    for s in (-1, 1.5, dict(lam=0.5), dict(iterations=1, lam=2)):
        with pytest.raises(ValueError):
            TS.fuse(None, kf, (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), smooth=s)
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels = Ctx(), 2, 1000
    for s in (-1, dict(iterations=1, mu=-3)):
        with pytest.raises(ValueError):
            vol.extract(1, smooth=s)
    vol._h = None


def test_nothing_is_imported_without_the_option():
    code = ("import sys; sys.path[:0] = [%r, %r]; from rgbid import tsdf as TS; assert TS.smooth_arg(None) is None; "
            "assert 'rgbid.smooth' not in sys.modules; TS.smooth_arg(3); assert 'rgbid.smooth' in sys.modules") % (
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
    src = tmp_path / "use_smooth.c"
    src.write_text('#include "rgbid_smooth.h"\n'
                   "int use(rgbid_smooth* h, rgbid_ctx* ctx, const float* v, const uint32_t* tris, float* vo, float* no, uint32_t* off, uint32_t* nb,\n"
                   "        uint32_t* inc, uint8_t* bd) {\n"
                   "  unsigned long long counts[8]; float ms[3];\n"
                   "  return rgbid_smooth_create(&h, ctx, RGBID_SMOOTH_MAX_VERTICES, RGBID_SMOOTH_MAX_TRIANGLES)\n"
                   "       + rgbid_smooth_plan(h, 10, 5, tris, RGBID_SMOOTH_PLAN_NORMALS, counts)\n"
                   "       + rgbid_smooth_adjacency(h, off, nb, inc, bd, counts[0])\n"
                   "       + rgbid_smooth_run(h, v, vo, RGBID_SMOOTH_MAX_ITERATIONS, 0.5, -0.53, RGBID_SMOOTH_PIN_BOUNDARY)\n"
                   "       + rgbid_smooth_normals(h, vo, no) + rgbid_smooth_timing(h, 1, ms) + rgbid_smooth_destroy(h); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_smooth.h")).read()
    assert int(re.search(r"RGBID_SMOOTH_MAX_VERTICES\s+(\d+)ull", txt).group(1)) == SO.MAX_VERTICES == 1 << 31
    assert int(re.search(r"RGBID_SMOOTH_MAX_TRIANGLES\s+(\d+)ull", txt).group(1)) == SO.MAX_TRIANGLES == 1 << 29
    assert int(re.search(r"RGBID_SMOOTH_MAX_ITERATIONS\s+(\d+)u", txt).group(1)) == SO.MAX_ITERATIONS == 4096
    assert int(re.search(r"RGBID_SMOOTH_PLAN_NORMALS\s+(\d+)u", txt).group(1)) == SO.PLAN_NORMALS
    assert int(re.search(r"RGBID_SMOOTH_PIN_BOUNDARY\s+(\d+)u", txt).group(1)) == SO.PIN_BOUNDARY


def test_library_exports_smooth_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_smooth.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_smooth_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(SO.EXPORTS) and len(declared) == 7, set(declared) ^ set(SO.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    L.rgbid_smooth_create.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_ulonglong]
    L.rgbid_smooth_plan.argtypes = [c.c_void_p, c.c_ulonglong, c.c_ulonglong, c.c_void_p, c.c_uint32, c.c_void_p]
    L.rgbid_smooth_adjacency.argtypes = [c.c_void_p] * 5 + [c.c_ulonglong]
    L.rgbid_smooth_run.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint, c.c_double, c.c_double, c.c_uint32]
    L.rgbid_smooth_normals.argtypes = [c.c_void_p] * 3
    L.rgbid_smooth_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_smooth_destroy.argtypes = [c.c_void_p]
    h = c.c_void_p()
    assert L.rgbid_smooth_create(c.byref(h), None, 10, 10) == -1 and not h.value and L.rgbid_smooth_create(None, None, 10, 10) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        assert L.rgbid_smooth_create(c.byref(h), fake, v, t) == -1 and not h.value
    assert L.rgbid_smooth_plan(None, 0, 0, None, 0, None) == -1
    assert L.rgbid_smooth_adjacency(None, None, None, None, None, 0) == -1
    assert L.rgbid_smooth_run(None, None, None, 1, 0.5, -0.53, 0) == -1 and L.rgbid_smooth_normals(None, None, None) == -1
    assert L.rgbid_smooth_timing(None, 0, None) == -1 and L.rgbid_smooth_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-smooth", "5"], "--mesh-smooth needs --mesh"),
                      (mesh_opt + ["--mesh-smooth-lambda", "0.5", "--mesh-smooth-mu", "-0.5"], "need --mesh-smooth"),
                      (mesh_opt + ["--mesh-smooth-pin-boundary"], "need --mesh-smooth"),
                      (mesh_opt + ["--mesh-smooth", "4097"], "iterations must lie in"), (mesh_opt + ["--mesh-smooth", "x"], "invalid int value"),
                      (mesh_opt + ["--mesh-smooth", "3", "--mesh-smooth-lambda", "nan"], "lam must be"),
                      (mesh_opt + ["--mesh-smooth", "3", "--mesh-smooth-mu", "0.1"], "mu must be")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()


def test_smoothed_mesh_through_the_ply_writer(tmp_path):
    m = all_cases()["sphere"]
    v = smoothed("sphere", 10)
    n = SM.normals(v, adjacency_of("sphere"))
    col = np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8)
    path = tmp_path / "smoothed.ply"
    TS.write_mesh_ply(str(path), v, col, m["triangles"], n)
    pv, pc, pt, pn = TS.read_mesh_ply(path.read_bytes())
    assert pv.tobytes() == v.tobytes() and pc.tobytes() == col.tobytes() and pt.tobytes() == m["triangles"].tobytes()
    assert pn.tobytes() == n.tobytes() and len(pt) == 4000 and len(pv) == 2002
