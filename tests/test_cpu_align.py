"""CPU checks of the alignment of depth frames to the TSDF volume (include/rgbid_tsdf_align.h, rgbid.tsdf): the numpy restatement the GPU
tests compare the kernels against (tests/align_mirror.py) against the plain scalar loop of the contract; the fixed sum tree against an
explicit loop; convergence on the prototype scene of DESIGN.md section 21; the threshold scene of the GPU tests, every case asserted on the
mirror; the Python argument checks one by one; the header as C99; the library's exports; the command line's option errors."""
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
from tests import align_mirror as AM
from tests import tsdf_mirror as TM
from tests.test_cpu_consist import COLS, DENORMAL, K, ROWS, cameras, surface_z
from tests.test_cpu_raycast import th_volume
from tests.test_cpu_tsdf import GATE, TH_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32
PROTO_GRID = dict(nx=64, ny=48, nz=32, origin=(-1.6, -1.2, 1.0), voxel=0.05, trunc=0.2)


# ---- the prototype scene ----------------------------------------------------------------------------------------------------------------
def exact_planes(R, t, rows=ROWS, cols=COLS, K_=K):
    """the inverse-depth planes of the surface of tests/test_cpu_consist.py seen from the world poses R, t: every pixel's ray is cut with
    z = surface_z(x, y) by Newton's iteration in double"""
    fx, fy, cx, cy = K_
    pu, pv = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    d = np.stack([(pu - cx) / fx, (pv - cy) / fy, np.ones_like(pu)], -1)
    out = []
    for v in range(len(R)):
        w = d @ np.asarray(R[v]).T
        z = np.full(pu.shape, 1.8)
        for _ in range(40):
            p = t[v] + w * z[..., None]
            s = surface_z(p[..., 0], p[..., 1])
            sx = (surface_z(p[..., 0] + 1e-6, p[..., 1]) - s) / 1e-6
            sy = (surface_z(p[..., 0], p[..., 1] + 1e-6) - s) / 1e-6
            z = z - (p[..., 2] - s) / (w[..., 2] - sx * w[..., 0] - sy * w[..., 1])
        p = t[v] + w * z[..., None]
        assert np.abs(p[..., 2] - surface_z(p[..., 0], p[..., 1])).max() < 1e-9
        out.append((1.0 / z).astype(F))
    return np.stack(out)


def perturbed(R, t, rad, metres, seed):
    """every pose turned by `rad` about a random axis and moved by `metres` in a random direction, both in the world frame"""
    rng = np.random.default_rng(seed)
    Rp, tp = [], []
    for v in range(len(R)):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        d = rng.normal(size=3); d *= metres / np.linalg.norm(d)
        Rp.append((np.eye(3) + np.sin(rad) * Kx + (1 - np.cos(rad)) * Kx @ Kx) @ R[v]); tp.append(t[v] + d)
    return np.stack(Rp), np.stack(tp)


@functools.lru_cache(maxsize=None)
def proto_scene(V=6, rows=ROWS, cols=COLS):
    """DESIGN.md section 21's scene: V views of the surface (2 % of the pixels are holes of every kind) fused into 64 x 48 x 32 voxels of
    0.05 m -> dict(R, t, planes, vol).  The views beyond the first six are not fused: they are frames of another run."""
    rng = np.random.default_rng(2100)
    R, t = cameras(rng, V)
    planes = exact_planes(R, t, rows, cols)
    kinds = np.array([NAN, 0.0, -0.5, INF, DENORMAL], F)
    hole = rng.random(planes.shape) < 0.02
    planes[hole] = kinds[rng.integers(0, len(kinds), int(hole.sum()))]
    vol = TM.Volume(**PROTO_GRID)
    n = min(V, 6)
    TM.integrate(vol, planes[:n], None, R[:n], t[:n], K, **GATE)
    return dict(R=R, t=t, planes=planes, vol=vol)


def pose_errors(sc, res):
    return np.array([AM.correction(sc["R"][v], sc["t"][v], res["pose"][v, :9].reshape(3, 3), res["pose"][v, 9:]) for v in range(len(res))])


# ---- mirror against the scalar loops ----------------------------------------------------------------------------------------------------
def test_mirror_equals_the_scalar_loop():
    sc = proto_scene()
    Rp, tp = perturbed(sc["R"][:2], sc["t"][:2], 0.04, 0.05, 7)
    a = AM.align(sc["vol"], sc["planes"], Rp, tp, K, ROWS, COLS, ((1, 3),), huber=0.03, **GATE)
    b = AM.align_loop(sc["vol"], sc["planes"], Rp, tp, K, ROWS, COLS, ((1, 3),), huber=0.03, **GATE)
    assert a.tobytes() == b.tobytes()
    assert (a["iterations"] == 3).all() and (a["used"] > 2000).all() and (a["pose"][:, :9].reshape(2, 3, 3) != Rp).any()
    px = AM.pixel_values(sc["vol"], sc["planes"][0], AM.pose32(np.concatenate([Rp[0].reshape(9), tp[0]])), K, ROWS, COLS, 1, 0.3, 5.0, 1, 0.03)
    assert 0 < (px["w"][px["used"]] < 1).sum() < px["used"].sum()        # both branches of the weight


def test_tree64_and_the_upper_tree_equal_explicit_loops():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(3, 64)) * 10.0 ** rng.integers(-8, 8, (3, 64))
    assert [float(x) for x in AM.tree64(v)] == [AM.tree64_loop(row) for row in v]
    # a ragged lattice: 13 x 21 pixels are 2 x 3 tiles; lane (ly & 7) 8 + (lx & 7), zeros outside
    x = rng.normal(size=(13, 21))
    lanes = AM.tile_lanes(x)
    assert lanes.shape == (6, 64)
    for tile in range(6):
        for lane in range(64):
            lx, ly = (tile % 3) * 8 + (lane & 7), (tile // 3) * 8 + (lane >> 3)
            want = x[ly, lx] if lx < 21 and ly < 13 else 0.0
            assert lanes[tile, lane] == want and (want != 0.0 or not np.signbit(lanes[tile, lane]))
    # tile counts 1, 64, 65 (not a multiple of 64), 300 (two rounds) and 4 800 (three)
    for n in (1, 2, 64, 65, 300, 4800):
        s = rng.normal(size=n) * 10.0 ** rng.integers(-6, 6, n)
        assert float(AM.reduce_tiles(s)) == AM.reduce_loop(s), n
    assert float(AM.reduce_tiles(np.array([-0.0]))) == 0.0 and np.signbit(AM.reduce_tiles(np.array([-0.0])))   # one tile: no round, no + 0.0
    s = np.array([1e16, 1.0, -1e16, 1.0] + [0.0] * 60)
    assert float(AM.reduce_tiles(s)) == 0.0 and float(np.sum(s[[0, 2, 1, 3]])) == 2.0                        # the tree's order, not another


# ---- convergence --------------------------------------------------------------------------------------------------------------------------
def test_converges_on_the_prototype_scene():
    """the figures of DESIGN.md section 21.  At the true poses 2 489 .. 3 010 pixels are used and the residual rms is 0.9 .. 1.2 mm.  From
    0.04 rad / 0.05 m, one level of 30 iterations at stride 1: the final errors are 0.0002 .. 0.0108 rad and 0.0008 .. 0.0070 m, their
    medians 0.0026 rad and 0.0027 m; five views converge after 10 .. 25 iterations and one uses all 30."""
    sc = proto_scene()
    at = AM.align(sc["vol"], sc["planes"], sc["R"], sc["t"], K, ROWS, COLS, ((1, 1),), **GATE)
    rms = np.sqrt(at["sums"][:, 0, 27] / at["used"][:, 0])
    print("true poses: used", at["used"][:, 0], "rms", rms, "cond(H)", [round(np.linalg.cond(AM.unpack(at["sums"][v, 0])[0])) for v in range(6)])
    assert (at["used"][:, 0] > 2000).all() and (rms < 0.002).all()
    Rp, tp = perturbed(sc["R"], sc["t"], 0.04, 0.05, 7)
    res = AM.align(sc["vol"], sc["planes"], Rp, tp, K, ROWS, COLS, ((1, 30),), **GATE)
    e = pose_errors(sc, res)
    print("status", res["status"], "iterations", res["iterations"], "errors (rad, m)", e.tolist(), "medians", np.median(e, 0))
    assert (e[:, 0] < 0.04).all() and (e[:, 1] < 0.05).all()                  # every view ends nearer than it began
    assert np.median(e[:, 0]) <= 0.01 and np.median(e[:, 1]) <= 0.0125        # the median: a quarter of the perturbation at most
    assert set(res["status"]) <= {AM.RUNNING, AM.CONVERGED} and (res["status"] == AM.CONVERGED).any()
    # the residual falls: the last system's error is below the first's
    assert (res["sums"][:, 1, 27] < res["sums"][:, 0, 27]).all()


# ---- the threshold scene: everything exact in float32 ---------------------------------------------------------------------------------
# th_volume() of tests/test_cpu_raycast.py: voxel = trunc = 1 / 8, centres at multiples of 1 / 8, D = clip(2 - z, +-1 / 8), W = 1 up to
# z = 2.125.  Every pixel of TH_PLANE measures z = 2 exactly; an identity camera moved by t puts pixel (pu, pv) at
# ((pu - 31.5) / 32 + tx, (pv - 23.5) / 32 + ty, 2 + tz): G = (0, 0, -1) wherever the sample is defined.
TH_PLANE = np.full((ROWS, COLS), 0.5, F)
TH_HOLES = TH_PLANE.copy()
TH_HOLES[0, :5] = [NAN, 0.0, -0.5, INF, DENORMAL]
TH_PARAMS = dict(z_min=1.5, z_max=2.5, huber=0.125, min_weight=1, min_pixels=6, levels=((1, 2),))
E = np.eye(3)
TH_ALIGN_CASES = {
    "edges": dict(TH_PARAMS, views=[(TH_PLANE, E, (-2.0 ** -6, 0, 0)),                  # gx of column 0 is 0 exactly: defined
                                    (TH_PLANE, E, (-2.0 ** -6 - 2.0 ** -23, 0, 0)),      # px one ulp below -1: undefined
                                    (TH_PLANE, E, (2.0 ** -6, 0, 0)),                   # gx of column 63 is nx - 1 = 16 exactly: undefined
                                    (TH_PLANE, E, (2.0 ** -6 - 2.0 ** -23, 0, 0))]),     # one ulp of px + 1 below: defined
    "trunc": dict(TH_PARAMS, views=[(TH_PLANE, E, (0, 0, -0.125)),                      # f = trunc exactly: free space, unused
                                    (TH_PLANE, E, (0, 0, -0.125 + 2.0 ** -23))]),        # f = trunc - 2^-23: used
    "huber": dict(TH_PARAMS, huber=0.0625, views=[(TH_PLANE, E, (0, 0, -0.0625)),       # |f| = huber: w = 1
                                                  (TH_PLANE, E, (0, 0, -0.0625 - 2.0 ** -23))]),   # one ulp above: w < 1
    "zmin_on": dict(TH_PARAMS, z_min=2.0, views=[(TH_PLANE, E, (0, 0, 0))]),
    "zmin_out": dict(TH_PARAMS, z_min=float(np.nextafter(F(2), F(3))), views=[(TH_PLANE, E, (0, 0, 0))]),
    "zmax_on": dict(TH_PARAMS, z_max=2.0, views=[(TH_PLANE, E, (0, 0, 0))]),
    "zmax_out": dict(TH_PARAMS, z_max=float(np.nextafter(F(2), F(0))), views=[(TH_PLANE, E, (0, 0, 0))]),
    "holes": dict(TH_PARAMS, views=[(TH_HOLES, E, (0, 0, 0))]),
    "weight": dict(TH_PARAMS, kind="block", min_weight=2, views=[(TH_PLANE, E, (0, 0, 0))]),
    "enough": dict(TH_PARAMS, min_pixels=ROWS * COLS - 5, views=[(TH_HOLES, E, (0, 0, 0))]),        # used = min_pixels: solved, SINGULAR
    "few": dict(TH_PARAMS, min_pixels=ROWS * COLS - 4, views=[(TH_HOLES, E, (0, 0, 0))]),           # one fewer: FEW
}


def th_align(name, views=None):
    """a case of the threshold scene (or some of its views) -> (volume, planes, R, t, the arguments of align after cols)"""
    c = dict(TH_ALIGN_CASES[name])
    vw = c.pop("views")
    vw = vw if views is None else [vw[i] for i in views]
    vol = th_volume(c.pop("kind", "wall"))
    return vol, [v[0] for v in vw], np.stack([v[1] for v in vw]), np.array([v[2] for v in vw], np.float64), c


def th_pixels(name, view):
    vol, planes, R, t, c = th_align(name, [view])
    px = AM.pixel_values(vol, planes[0], AM.pose32(np.concatenate([R[0].reshape(9), t[0]])), TH_K, ROWS, COLS, 1, c["z_min"], c["z_max"],
                         c["min_weight"], c["huber"])
    return px, AM.align(vol, planes, R, t, TH_K, ROWS, COLS, **c)


def test_threshold_scene_hits_every_case():
    px, _ = th_pixels("edges", 0)
    assert (px["g"][0][:, 0] == 0).all() and px["used"].all()
    px, _ = th_pixels("edges", 1)
    assert (px["g"][0][:, 0] == -F(2.0 ** -20)).all() and not px["used"][:, 0].any() and px["used"][:, 1:].all()
    px, _ = th_pixels("edges", 2)
    assert (px["g"][0][:, 63] == 16).all() and not px["used"][:, 63].any() and px["used"][:, :63].all()      # the domain is half-open
    px, _ = th_pixels("edges", 3)
    assert (px["g"][0][:, 63] == F(16) - F(2.0 ** -20)).all() and px["used"].all()
    px, r = th_pixels("trunc", 0)
    assert (px["f"] == F(0.125)).all() and px["defined"].all() and not px["used"].any() and r["status"][0] == AM.FEW and r["used"][0, 0] == 0
    px, _ = th_pixels("trunc", 1)
    assert (px["f"] == F(0.125) - F(2.0 ** -23)).all() and px["used"].all()
    px, _ = th_pixels("huber", 0)
    assert (px["f"] == F(0.0625)).all() and (px["w"] == 1).all() and px["used"].all()
    px, _ = th_pixels("huber", 1)
    assert (px["f"] == F(0.0625) + F(2.0 ** -23)).all() and (px["w"] < 1).all() and (px["w"] > F(0.9999)).all()
    for name, used in (("zmin_on", True), ("zmin_out", False), ("zmax_on", True), ("zmax_out", False)):
        px, r = th_pixels(name, 0)
        assert (px["z"] == 2).all() and px["used"].all() == used and px["used"].any() == used, name
        assert r["status"][0] == (AM.SINGULAR if used else AM.FEW)
    px, r = th_pixels("holes", 0)
    assert not px["measured"][0, :5].any() and not px["used"][0, :5].any() and px["used"].sum() == ROWS * COLS - 5
    with np.errstate(all="ignore"):
        assert np.isfinite(TH_HOLES[0, 4]) and TH_HOLES[0, 4] > 0 and np.isinf(F(1) / TH_HOLES[0, 4])        # the denormal's reciprocal overflows
    px, r = th_pixels("weight", 0)
    assert px["used"].any() and not px["used"].all() and th_pixels("edges", 0)[0]["defined"].all()
    assert (px["used"] == (px["defined"] & (np.abs(px["f"]) < F(0.125)))).all()
    # used = min_pixels: the system is solved, and the flat wall's H has exact zero rows 0, 1 and 5: SINGULAR at the first pivot
    px, r = th_pixels("enough", 0)
    H, b, err = AM.unpack(r["sums"][0, 0])
    assert r["used"][0, 0] == ROWS * COLS - 5 == TH_ALIGN_CASES["enough"]["min_pixels"] and r["status"][0] == AM.SINGULAR and r["iterations"][0] == 1
    assert not H[[0, 1, 5]].any() and H[2, 2] == ROWS * COLS - 5 and H[3, 3] > 0 and H[4, 4] > 0 and err == 0 and not b.any()
    assert all((px["G"][i][px["used"]] == v).all() for i, v in enumerate((0, 0, -1)))
    vol, planes, R, t, c = th_align("enough")
    want = np.concatenate([R[0].reshape(9), t[0]])
    assert r["pose"][0].tobytes() == want.tobytes()
    px, r = th_pixels("few", 0)                                       # one fewer: FEW, and the pose bytes are the ones given
    assert r["status"][0] == AM.FEW and r["iterations"][0] == 1 and r["used"].tolist() == [[ROWS * COLS - 5] * 2] and r["pose"][0].tobytes() == want.tobytes()
    assert r["sums"][0, 0].tobytes() == r["sums"][0, 1].tobytes() and r["sums"][0, 0, 11] == ROWS * COLS - 5
    # every view alone gives the record it has in the common call
    for name in ("edges", "trunc", "huber"):
        vol, planes, R, t, c = th_align(name)
        all_ = AM.align(vol, planes, R, t, TH_K, ROWS, COLS, **c)
        for v in range(len(R)):
            assert th_pixels(name, v)[1].tobytes() == all_[v:v + 1].tobytes()


def test_levels_restart_converged_views_and_stopped_views_stay():
    sc = proto_scene()
    # a large eps: the view converges in the first level at once and runs again in the second
    r = AM.align(sc["vol"], sc["planes"], sc["R"][:1], sc["t"][:1], K, ROWS, COLS, ((2, 5), (1, 5)), eps=1.0, **GATE)
    assert r["status"][0] == AM.CONVERGED and r["iterations"][0] == 2
    r = AM.align(sc["vol"], sc["planes"], sc["R"][:1], sc["t"][:1], K, ROWS, COLS, ((2, 5), (1, 5)), min_pixels=4000, **GATE)
    assert r["status"][0] == AM.FEW and r["iterations"][0] == 1                # FEW is final: the second level does not run it


# ---- the Python checkers, one by one --------------------------------------------------------------------------------------------------
def test_levels_checker():
    assert TS.align_levels_arg(TS.ALIGN_LEVELS) == ((4, 10), (2, 10), (1, 10)) and TS.align_levels_arg([[8, 256]]) == ((8, 256),)
    assert TS.align_levels_arg(((1, 64),) * 4) == ((1, 64),) * 4
    for bad in ((), ((1, 1),) * 5, ((3, 1),), ((0, 1),), ((16, 1),), ((1, 0),), ((1, -1),), ((1, 257),), ((1, 200), (2, 57)), ((1.0, 1),), ((1, 2.0),),
                ((1,),), ((1, 2, 3),), 5, None, ((True, 1),)):
        with pytest.raises(ValueError):
            TS.align_levels_arg(bad)


def test_params_checker():
    assert TS.align_params_arg(0.2, 0, 1e-6, 6) == (float(F(0.2)), 0.0, 1e-6, 6)
    assert TS.align_params_arg(np.float32(0.01), 1e-3, 1.0, 1 << 20)[3] == 1 << 20
    for bad in (dict(huber=0), dict(huber=-1), dict(huber=NAN), dict(huber=INF), dict(huber=1e39), dict(huber="x"), dict(huber=None),
                dict(damping=-1e-9), dict(damping=NAN), dict(damping=INF), dict(damping="x"), dict(eps=0), dict(eps=-1e-6), dict(eps=NAN),
                dict(eps=INF), dict(eps=None), dict(min_pixels=5), dict(min_pixels=0), dict(min_pixels=-1), dict(min_pixels=64.0),
                dict(min_pixels=1 << 32), dict(min_pixels=True)):
        a = dict(huber=0.2, damping=0.0, eps=1e-6, min_pixels=64)
        a.update(bad)
        with pytest.raises(ValueError):
            TS.align_params_arg(**a)


def test_checks_come_before_the_library():
    class Ctx:
        device = 0
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels, vol.voxel, vol.trunc = Ctx(), 2, 1000, 0.05, 0.2
    good = dict(planes=None, R=np.eye(3), t=np.zeros(3), K=K, rows=ROWS, cols=COLS)
    for change in (dict(z_min=0.0), dict(z_min=3.0, z_max=2.0), dict(z_max=INF), dict(K=(0, 58, 31.5, 23.5)), dict(K=(60, 0, 31.5, 23.5)),
                   dict(K=(60, 58, NAN, 23.5)), dict(t=[NAN, 0, 0]), dict(R=np.full((3, 3), 1e300)), dict(rows=0), dict(cols=(1 << 20) + 1),
                   dict(rows=1 << 16, cols=1 << 15), dict(R=np.zeros((0, 3, 3)), t=np.zeros((0, 3))), dict(R=np.stack([np.eye(3)] * 3), t=np.zeros((3, 3))),
                   dict(min_weight=0), dict(min_weight=65536), dict(min_weight=1.0), dict(huber=0.0), dict(huber=NAN), dict(damping=-1.0),
                   dict(eps=0.0), dict(min_pixels=5), dict(levels=()), dict(levels=((3, 1),)), dict(levels=((1, 257),)),
                   dict(planes=[np.zeros((ROWS, COLS), F)]), dict(planes=5)):                              # planes that are no CUDA tensors
        with pytest.raises(ValueError):
            vol.align(**dict(good, **change))
    with pytest.raises(ValueError):
        vol.align_into(None, np.eye(3), np.zeros(3), K, ROWS, COLS, TS.ALIGN_LEVELS, 0.2, 0.0, 1e-6, 64, 1, 0.05, 20.0, result=np.zeros(560, np.uint8))
    with pytest.raises(ValueError):
        TS.align_check(None, [dict()], K, ROWS, COLS)                      # a model and a frame to align need two keyframes
    vol._h = None                                           # nothing to destroy


def test_result_record_and_summaries():
    assert TS.ALIGN_RESULT == AM.RESULT_DTYPE and TS.ALIGN_RESULT.itemsize == 560 and TS.ALIGN_STATUS == AM.STATUS_NAMES
    sc = proto_scene()
    res = AM.align(sc["vol"], sc["planes"], sc["R"][:2], sc["t"][:2], K, ROWS, COLS, ((2, 2),), **GATE)
    d, m = TS.align_dict(res), AM.as_dict(res)
    assert all(d[k].tobytes() == m[k].tobytes() for k in m) and set(d) == set(m)
    assert d["H"].shape == (2, 2, 6, 6) and (d["H"] == d["H"].transpose(0, 1, 3, 2)).all() and d["H"][0, 0, 1, 4] == res["sums"][0, 0, 9]
    rot, tr = TS.pose_correction(np.eye(3), np.zeros(3), perturbed(np.eye(3)[None], np.zeros((1, 3)), 0.03, 0.07, 1)[0][0], [0.07, 0, 0])
    assert abs(rot - 0.03) < 1e-12 and abs(tr - 0.07) < 1e-15
    figures = [dict(rotation=0.01, translation=0.02, status="converged"), dict(rotation=0.03, translation=0.01, status="few"),
               dict(rotation=0.02, translation=0.03, status="converged")]
    s = TS.align_check_summary(figures)
    assert s == dict(views=3, rotation_median=0.02, rotation_max=0.03, translation_median=0.02, translation_max=0.03,
                     status=dict(running=0, converged=2, few=1, singular=0))


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_align.c"
    src.write_text('#include "rgbid_tsdf.h"\n'
                   "int use(rgbid_tsdf* v, const rgbid_tsdf_view* views, rgbid_tsdf_align_result* result) {\n"
                   "  const float K[4] = {525.f, 525.f, 319.5f, 239.5f}; float ms[2];\n"
                   "  const rgbid_tsdf_align_level levels[3] = {{4, 10}, {2, 10}, {1, 10}};\n"
                   "  return rgbid_tsdf_align(v, 16, views, K, 480, 640, 0.05f, 20.f, 1u, 0.08f, 0.0, 1e-6, 64u, 3, levels, result)\n"
                   "       + rgbid_tsdf_align_timing(v, 1, ms) + (sizeof(rgbid_tsdf_align_result) == 560 ? 0 : 1)\n"
                   "       + (RGBID_TSDF_ALIGN_MAX_ITERATIONS == 256 && RGBID_TSDF_ALIGN_MAX_LEVELS == 4 && RGBID_TSDF_ALIGN_TERMS == 28 ? 0 : 1)\n"
                   "       + (RGBID_TSDF_ALIGN_SINGULAR == 3 ? 0 : 1); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_tsdf_align.h")).read()
    for name, want in (("MAX_LEVELS", TS.ALIGN_MAX_LEVELS), ("MAX_ITERATIONS", TS.ALIGN_MAX_ITERATIONS), ("TERMS", AM.TERMS)):
        assert int(re.search(r"RGBID_TSDF_ALIGN_%s\s+(\d+)" % name, txt).group(1)) == want
    for k, word in enumerate(("RUNNING", "CONVERGED", "FEW", "SINGULAR")):
        assert int(re.search(r"RGBID_TSDF_ALIGN_%s = (\d+)" % word, txt).group(1)) == k == getattr(AM, word) and TS.ALIGN_STATUS[k] == word.lower()
    tail = open(os.path.join(ROOT, "include", "rgbid_tsdf.h")).read()
    assert tail.index('#include "rgbid_tsdf_raycast.h"') < tail.index('#include "rgbid_tsdf_align.h"')


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_align_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_tsdf_align.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_tsdf_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(TS.ALIGN_EXPORTS) and len(declared) == 2, set(declared) ^ set(TS.ALIGN_EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    L.rgbid_tsdf_align.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_float, c.c_float, c.c_uint, c.c_float,
                                   c.c_double, c.c_double, c.c_uint, c.c_int, c.c_void_p, c.c_void_p]
    L.rgbid_tsdf_align_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    view, k, lv = TS.View(), (c.c_float * 4)(*K), (c.c_int * 2)(1, 1)
    assert L.rgbid_tsdf_align(None, 1, c.byref(view), k, ROWS, COLS, 0.3, 5.0, 1, 0.2, 0.0, 1e-6, 64, 1, lv, None) == -1
    assert L.rgbid_tsdf_align_timing(None, 0, None) == -1


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-align-check"], "need --mesh"), (["--mesh-align-iterations", "5"], "need --mesh"),
                      (mesh + ["--mesh-align-iterations", "5"], "needs --mesh-align-check"),
                      (mesh + ["--mesh-align-check", "--mesh-align-iterations", "0"], "at least 1 iteration"),
                      (mesh + ["--mesh-align-check", "--mesh-align-iterations", "86"], "at most 256"),
                      (mesh + ["--mesh-align-check", "--mesh-align-iterations", "x"], "invalid int value")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()
