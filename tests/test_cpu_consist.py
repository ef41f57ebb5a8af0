"""CPU checks of the consistency filter (include/rgbid_consist.h, rgbid.consist): the numpy restatement the GPU tests compare the kernels
against (tests/consist_mirror.py) against the plain scalar loop of the contract; scenes whose counts are derived by hand; the Python
argument checks one by one; the header as C99; the library's exports; refusals that need no device; the command line's option errors."""
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
from rgbid import cloud as CL
from rgbid import consist as CF
from tests import consist_mirror as CM
from tests import render_mirror as RM
from tests.test_cpu_render import cloud_around, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32
ROWS, COLS = 48, 64
K = (60.0, 58.0, 31.5, 23.5)
DENORMAL = F(1e-39)                     # 1.f / 1e-39f overflows: finite and > 0, yet not measured


def surface_z(x, y):
    """a smooth surface in front of cameras near the origin that look along +z"""
    return 1.8 + 0.25 * np.sin(1.3 * x) * np.cos(0.9 * y) + 0.1 * x


def surface_cloud(rng, n, half=2.2):
    p = np.zeros(n, CL.POINT_DTYPE)
    x, y = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
    p["x"], p["y"], p["z"] = x.astype(F), y.astype(F), surface_z(x, y).astype(F)
    return p


def surface_planes(rng, R, t, rows=ROWS, cols=COLS, K_=K, holes=0.08):
    """each view's inverse-depth plane: the surface rendered by the renderer's mirror, 1 / depth, NaN where nothing was drawn, and holes
    of every kind the contract names: NaN, 0, negative, +inf and a denormal whose reciprocal is infinite"""
    depth = RM.render_numpy(surface_cloud(rng, 30_000), R, t, K_, rows, cols, 1, 0.05, 20.0)["depth"]
    with np.errstate(all="ignore"):
        iD = (F(1) / depth).astype(F)
    kinds = np.array([NAN, 0.0, -0.5, INF, DENORMAL], F)
    hole = rng.random(iD.shape) < holes
    iD[hole] = kinds[rng.integers(0, len(kinds), int(hole.sum()))]
    return iD


def cameras(rng, V):
    """the first at the origin with the identity pose (Z = z exactly), the others moved and turned a little"""
    R = np.stack([np.eye(3)] + [rotation(rng, 0.35) for _ in range(V - 1)])
    t = np.concatenate([np.zeros((1, 3)), rng.uniform(-0.35, 0.35, (V - 1, 3))])
    return R, t


def records_near_surface(rng, n):
    """cloud_around's box (NaN and inf positions included) with two thirds of the records moved to the surface, scaled along their ray by
    0.9 .. 1.1: some within the tolerance, some in front, some behind"""
    p = cloud_around(rng, n, depth=(0.3, 3.0), half=1.2)
    on = rng.random(n) < 0.66
    x, y = p["x"].astype(np.float64), p["y"].astype(np.float64)
    s = rng.choice([1.0, 1.0, 0.99, 1.01, 0.9, 1.1, 0.97, 1.03], n)
    with np.errstate(invalid="ignore"):
        z = surface_z(x, y)
        for c, v in (("x", x * s), ("y", y * s), ("z", z * s)):
            p[c] = np.where(on & np.isfinite(p[c]), v.astype(F), p[c])
    return p


HALF = 524288                           # one full grid of the strided kernels and 256 tiles of the keep compaction (test_cpu_segment.py
LARGE_N = 2 * HALF + 5003               # test_sizes_lie_on_the_intended_side_of_the_thresholds): three trips, the last one ragged
LARGE_GATE = dict(tol_rel=0.02, tol_abs=0.001, window=1, z_min=0.3, z_max=5.0)


@functools.lru_cache(maxsize=None)
def large_cloud():
    """LARGE_N records around the surface, 1 % of them with y = -inf, and VIEW_CHUNK + 1 cameras with their planes; tests/test_gpu_consist.py
    filters prefixes of it against the first three views and against all of them"""
    rng = np.random.default_rng(500)
    R, t = cameras(rng, CF.VIEW_CHUNK + 1)
    planes = surface_planes(rng, R, t)
    p = records_near_surface(rng, LARGE_N)
    p["y"][rng.random(len(p)) < 0.01] = -np.inf
    return dict(p=p, R=R, t=t, planes=planes)


def assert_every_trip_has_work(sup, con, keep, pairs, n):
    """a trip of the stride that did nothing must not pass: the records of each trip include supported, contradicted and removed ones"""
    assert keep.sum() > n // 2 and (sup > 0).sum() > n // 8 and (con > 0).sum() > n // 16 and pairs > n // 2
    for lo in range(0, n, HALF):
        hi = min(lo + HALF, n)
        few = min(hi - lo, 5003) // 50                     # 100 of each kind, unless the trip has fewer than 5 003 records
        assert (sup[lo:hi] > 0).sum() >= few and (con[lo:hi] > 0).sum() >= few and (~keep[lo:hi]).sum() >= few, (lo, hi)


def test_large_cloud_has_work_on_every_trip():
    sc = large_cloud()
    counts, keep, kept, pairs = CM.consist_numpy(sc["p"], None, sc["planes"][:3], sc["R"][:3], sc["t"][:3], K, **LARGE_GATE)
    sup, con = unpack(counts)
    print(f"{LARGE_N} records, 3 views: {int(keep.sum())} kept, {int((sup > 0).sum())} supported, {int((con > 0).sum())} contradicted, {pairs} pairs")
    assert_every_trip_has_work(sup, con, keep, pairs, LARGE_N)
    assert len(kept) == keep.sum() < LARGE_N


def unpack(counts):
    c = np.asarray(counts).view(np.uint32)
    return (c & 0xFFFF).astype(np.int64), (c >> 16).astype(np.int64)


@pytest.mark.parametrize("w", [0, 1, 2])
def test_mirror_equals_the_scalar_loop(w):
    rng = np.random.default_rng(40 + w)
    V, n = 4, 500
    R, t = cameras(rng, V)
    planes = surface_planes(rng, R, t)
    p = records_near_surface(rng, n)
    off = np.array([0, 120, 120, 330, n])                  # an empty owner range among them
    for offsets in (None, off):
        counts, keep, kept, pairs = CM.consist_numpy(p, offsets, planes, R, t, K, 0.02, 0.001, w, 1, 0, 0.3, 5.0)
        sup, con = CM.consist_loop(p, offsets, planes, R, t, K, 0.02, 0.001, w, 0.3, 5.0)
        gs, gc = unpack(counts)
        assert np.array_equal(gs, sup) and np.array_equal(gc, con)
        part = np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])
        assert np.array_equal(keep, part & (sup >= 1) & (con <= 0)) and kept.tobytes() == p[keep].tobytes()
        assert sup.max() >= 2 and con.max() >= 1 and 0 < keep.sum() < part.sum() < n and pairs > n


def analytic_scene():
    """three identity-rotation cameras before a wall at z = 2 (iD = 0.5 everywhere); 30 records on the wall, 10 in front of it at z = 1,
    10 behind it at z = 3, all inside every camera's image"""
    rng = np.random.default_rng(1)
    p = np.zeros(50, CL.POINT_DTYPE)
    p["x"][:30], p["y"][:30], p["z"][:30] = rng.uniform(-0.3, 0.3, 30), rng.uniform(-0.2, 0.2, 30), 2
    p["x"][30:40], p["y"][30:40], p["z"][30:40] = rng.uniform(-0.1, 0.1, 10), rng.uniform(-0.1, 0.1, 10), 1
    p["x"][40:], p["y"][40:], p["z"][40:] = rng.uniform(-0.3, 0.3, 10), rng.uniform(-0.2, 0.2, 10), 3
    p["r"] = np.arange(50)
    R = np.stack([np.eye(3)] * 3)
    t = np.array([[0, 0, 0], [0.25, 0, 0], [-0.125, 0.0625, 0]], np.float64)
    planes = np.full((3, ROWS, COLS), 0.5, F)
    return p, R, t, planes


@pytest.mark.parametrize("w", [0, 1, 2])
def test_analytic_scene(w):
    """on the wall: every camera measured 2 m where the record is, |e| = 0: support 3.  In front: every camera measured 2 m behind a
    record at 1 m, e = 1 > 0.02: conflicts 3.  Behind: e = -1, occluded, blind.  An owner is no witness of its own records."""
    p, R, t, planes = analytic_scene()
    gate = dict(tol_rel=0.02, tol_abs=0.0, window=w, z_min=0.3, z_max=5.0)
    counts, keep, kept, pairs = CM.consist_numpy(p, None, planes, R, t, K, **gate)
    sup, con = unpack(counts)
    assert (sup[:30] == 3).all() and (con[:30] == 0).all()
    assert (sup[30:40] == 0).all() and (con[30:40] == 3).all()
    assert (sup[40:] == 0).all() and (con[40:] == 0).all()
    assert pairs == 150
    assert np.array_equal(keep, np.r_[np.ones(30, bool), np.zeros(10, bool), np.ones(10, bool)])       # the defaults: the 10 in front go
    assert np.array_equal(kept["r"], np.r_[np.arange(30), np.arange(40, 50)])
    counts, keep, _, pairs = CM.consist_numpy(p, [0, 30, 40, 50], planes, R, t, K, **gate)
    sup, con = unpack(counts)
    assert (sup[:30] == 2).all() and (con[:30] == 0).all() and (sup[30:40] == 0).all() and (con[30:40] == 2).all()
    assert not sup[40:].any() and not con[40:].any() and pairs == 100
    _, keep, _, _ = CM.consist_numpy(p, None, planes, R, t, K, min_support=1, **gate)
    assert keep[:30].all() and not keep[30:].any()         # with min_support = 1 the 10 behind go as well
    ls, lc = CM.consist_loop(p, None, planes, R, t, K, 0.02, 0.0, w, 0.3, 5.0)
    assert ls.tolist() == [3] * 30 + [0] * 20 and lc.tolist() == [0] * 30 + [3] * 10 + [0] * 10


def test_step_scene_for_the_window():
    """the plane steps from 2 m to 1 m between columns 31 and 32; a record at 1 m projects to column 31: alone (w = 0) that pixel measured
    2 m behind it, a contradiction; with its neighbours (w = 1) the 1 m of column 32 supports it"""
    p = np.zeros(1, CL.POINT_DTYPE)
    p["x"], p["y"], p["z"] = F(-0.5 / 60), 0, 1
    plane = np.full((1, ROWS, COLS), 0.5, F)
    plane[0, :, 32:] = 1.0
    m = RM.pose_cw(np.eye(3), np.zeros(3))
    _, pu, pv, _ = RM.visible(p, m, K, ROWS, COLS, 0, 0.3, 5.0)
    assert pu.tolist() == [31] and pv.tolist() == [24]
    for w, want in ((0, (0, 1)), (1, (1, 0)), (2, (1, 0))):
        counts, keep, _, _ = CM.consist_numpy(p, None, plane, np.eye(3)[None], np.zeros((1, 3)), K, 0.02, 0.0, w, 0, 0, 0.3, 5.0)
        assert (int(counts[0]) & 0xFFFF, int(counts[0]) >> 16) == want and bool(keep[0]) == (want[1] == 0)
        sup, con = CM.consist_loop(p, None, plane, np.eye(3)[None], np.zeros((1, 3)), K, 0.02, 0.0, w, 0.3, 5.0)
        assert (sup[0], con[0]) == want


def test_holes_are_not_measured():
    ok, zm = CM.measured_depth(np.array([0.5, NAN, 0.0, -0.5, INF, DENORMAL, 1e-38], F))
    assert ok.tolist() == [True, False, False, False, False, False, True] and zm[0] == 2 and np.isinf(zm[5])
    # a window of holes only is blind, a window with one farther measurement among holes contradicts
    p = np.zeros(1, CL.POINT_DTYPE)
    p["z"] = 1
    plane = np.full((1, ROWS, COLS), NAN, F)
    args = (np.eye(3)[None], np.zeros((1, 3)), K, 0.02, 0.0, 1, 0, 0, 0.3, 5.0)
    assert int(CM.consist_numpy(p, None, plane, *args)[0][0]) == 0
    plane[0, 23, 31] = 0.5
    assert int(CM.consist_numpy(p, None, plane, *args)[0][0]) == 1 << 16
    plane[0, 25, 33] = 2.0                                 # and one nearer one: partly occluded, blind again
    assert int(CM.consist_numpy(p, None, plane, *args)[0][0]) == 0


def test_tolerances_checker():
    assert CF.tolerances(0.02) == (float(F(0.02)), 0.0) and CF.tolerances(0, 0) == (0.0, 0.0) and CF.tolerances(np.float32(0.5), 1) == (0.5, 1.0)
    for a, b in ((-0.01, 0), (0.02, -1e-3), (NAN, 0), (0.02, NAN), (INF, 0), (0.02, INF), (1e39, 0), ("a", 0), (None, 0), (0.02, None), ([1, 2], 0)):
        with pytest.raises(ValueError):
            CF.tolerances(a, b)


def test_window_checker():
    assert [CF.window_arg(w) for w in (0, 1, 2, np.int64(2))] == [0, 1, 2, 2]
    for w in (-1, 3, 1.0, "1", None, True):
        with pytest.raises(ValueError):
            CF.window_arg(w)


def test_vote_checker():
    assert CF.vote_args(0, 0) == (0, 0) and CF.vote_args(np.int32(3), 65535) == (3, 65535)
    for s, c in ((-1, 0), (0, -1), (65536, 0), (0, 65536), (1.0, 0), (0, "0"), (None, 0), (True, 0)):
        with pytest.raises(ValueError):
            CF.vote_args(s, c)


def test_offsets_checker():
    assert CF.offsets_arg(None, 3, 10) is None
    o = CF.offsets_arg([0, 4, 4, 10], 3, 10)
    assert o.dtype == np.uint64 and o.tolist() == [0, 4, 4, 10] and CF.offsets_arg(np.array([0, 0], np.uint64), 1, 0).tolist() == [0, 0]
    for off, V, n in (([0, 4, 10], 3, 10), ([1, 4, 4, 10], 3, 10), ([0, 5, 4, 10], 3, 10), ([0, 4, 4, 9], 3, 10), ([0, 4, 4, 11], 3, 10),
                      ([0.0, 4.0, 4.0, 10.0], 3, 10), ([-1, 0, 4, 10], 3, 10), ("abcd", 3, 10), ([[0, 4, 4, 10]], 3, 10)):
        with pytest.raises(ValueError):
            CF.offsets_arg(off, V, n)


def test_planes_checker_needs_cuda_float32_planes_of_the_image_size():
    import torch
    good = torch.zeros((ROWS, COLS), dtype=torch.float32)
    for planes, V in (([good], 1),                          # a host tensor
                      ([good.numpy()], 1), ([], 1), (None, 1), (good.to(torch.float64), 1), ([good, good], 3)):
        with pytest.raises(ValueError):
            CF.planes_arg(planes, V, ROWS, COLS)


def test_offsets_of_kept():
    counts = np.array([3, 0, 1 << 16, 2, (2 << 16) | 1, 0], np.uint32)
    assert CF.offsets_of_kept(counts, [0, 2, 2, 6]).tolist() == [0, 2, 2, 4]
    assert CF.offsets_of_kept(counts, [0, 2, 2, 6], min_support=1, max_conflicts=2).tolist() == [0, 1, 1, 3]
    assert CF.offsets_of_kept(counts.view(np.int32), [0, 2, 2, 6], finite=[True, False, True, True, True, True]).tolist() == [0, 1, 1, 3]


def test_filter_checks_come_before_the_library():
    class NoDevice:
        shape = (0, 32)
    good = dict(offsets=None, planes=[], R=np.eye(3), t=np.zeros(3), K=K, rows=ROWS, cols=COLS)
    for change in (dict(tol_rel=-1.0), dict(tol_abs=NAN), dict(window=3), dict(min_support=-1), dict(max_conflicts=1 << 16), dict(z_min=0.0),
                   dict(z_min=3.0, z_max=2.0), dict(K=(0, 58, 31.5, 23.5)), dict(t=[NAN, 0, 0]), dict(rows=0), dict(offsets=[0, 1]),
                   dict(R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)))):
        with pytest.raises(ValueError):
            CF.consistency_filter(None, NoDevice(), **dict(good, **change))


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_consist.c"
    src.write_text('#include "rgbid_consist.h"\n'
                   "typedef char view_is_a_pose_and_a_pointer[sizeof(rgbid_consist_view) == 96 + sizeof(void*) ? 1 : -1];\n"
                   "typedef char params_are_seven_words[sizeof(rgbid_consist_params) == 28 ? 1 : -1];\n"
                   "int use(rgbid_consist* c, const rgbid_cloud_point* p, const rgbid_consist_view* v, const unsigned long long* off, uint32_t* cnt,\n"
                   "        rgbid_cloud_point* out) {\n"
                   "  const float K[4] = {525.f, 525.f, 319.5f, 239.5f}; float ms[3]; unsigned long long st[4], kept;\n"
                   "  rgbid_consist_params prm = {0.02f, 0.f, RGBID_CONSIST_MAX_WINDOW, 0.05f, 20.f, 0u, 0u};\n"
                   "  return rgbid_consist_plan(c, p, 0, RGBID_CONSIST_MAX_VIEWS, v, off, K, 480, 640, &prm, st, &kept) + rgbid_consist_counts(c, cnt)\n"
                   "       + rgbid_consist_emit(c, out, kept) + rgbid_consist_timing(c, 1, ms); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_consist.h")).read()
    assert int(re.search(r"RGBID_CONSIST_MAX_POINTS\s+(\d+)ull", txt).group(1)) == CF.MAX_POINTS
    assert int(re.search(r"RGBID_CONSIST_MAX_VIEWS\s+(\d+)", txt).group(1)) == CF.MAX_VIEWS
    assert int(re.search(r"RGBID_CONSIST_MAX_WINDOW\s+(\d+)", txt).group(1)) == CF.MAX_WINDOW
    assert int(re.search(r"RGBID_CONSIST_MAX_DIM\s+(\d+)", txt).group(1)) == CF.MAX_DIM
    assert int(re.search(r"RGBID_CONSIST_VIEW_CHUNK\s+(\d+)", txt).group(1)) == CF.VIEW_CHUNK
    assert ctypes.sizeof(CF.View) == 104 and ctypes.sizeof(CF.Params) == 28


def test_library_exports_consist_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_consist.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_consist_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(CF.EXPORTS), set(declared) ^ set(CF.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    """argument checks come before the library touches the runtime: a null filter, a null context, capacities of 0 or past the bounds"""
    L = _lib_handle()
    L.rgbid_consist_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int]
    L.rgbid_consist_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.rgbid_consist_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.rgbid_consist_emit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong]
    L.rgbid_consist_timing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    h = ctypes.c_void_p()
    assert L.rgbid_consist_create(ctypes.byref(h), None, 10, 2) == -1 and not h.value
    assert L.rgbid_consist_create(None, None, 10, 2) == -1
    view = CF.View()
    prm = CF.Params(0.02, 0.0, 1, 0.05, 20.0, 0, 0)
    k = (ctypes.c_float * 4)(*K)
    kept = ctypes.c_ulonglong()
    assert L.rgbid_consist_plan(None, None, 0, 1, ctypes.byref(view), None, k, ROWS, COLS, ctypes.byref(prm), None, ctypes.byref(kept)) == -1
    assert L.rgbid_consist_counts(None, None) == -1 and L.rgbid_consist_emit(None, None, 0) == -1 and L.rgbid_consist_timing(None, 0, None) == -1
    assert L.rgbid_consist_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    ply = ["--cloud", str(tmp_path / "m.ply")]
    for bad, word in ((["--cloud-consistency", "0.02"], "--cloud-consistency needs --cloud"),
                      (ply + ["--cloud-consistency-abs", "0.01"], "need --cloud-consistency"),
                      (ply + ["--cloud-consistency-window", "1"], "need --cloud-consistency"),
                      (ply + ["--cloud-min-support", "1"], "need --cloud-consistency"),
                      (ply + ["--cloud-max-conflicts", "1"], "need --cloud-consistency"),
                      (ply + ["--cloud-consistency", "-0.02"], "tol_rel, tol_abs must be finite and >= 0"),
                      (ply + ["--cloud-consistency", "nan"], "tol_rel, tol_abs must be finite and >= 0"),
                      (ply + ["--cloud-consistency", "0.02", "--cloud-consistency-abs", "-1"], "tol_rel, tol_abs must be finite and >= 0"),
                      (ply + ["--cloud-consistency", "0.02", "--cloud-consistency-window", "3"], "window must lie in"),
                      (ply + ["--cloud-consistency", "0.02", "--cloud-min-support", "-1"], "min_support and max_conflicts must lie in"),
                      (ply + ["--cloud-consistency", "0.02", "--cloud-max-conflicts", "65536"], "min_support and max_conflicts must lie in")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()
