"""CPU checks of the map renderer (include/rgbid_render.h, rgbid.render): the numpy restatement the GPU tests compare the kernels against
(tests/render_mirror.py) against an independent per-pixel loop; the host half of the contract (the pose as twelve floats) against the
library; the Python argument checks; the header as C99; the library's exports; refusals that need no device; the command line."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from rgbid import _lib
from rgbid import cloud as CL
from rgbid import render as RD
from tests import render_mirror as RM
from tests.test_cpu_voxel import random_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32
K_TINY = (14.0, 13.0, 7.5, 5.5)


def rotation(rng, max_angle):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def cloud_around(rng, n, depth=(0.3, 3.0), half=1.6, nan=0.03):
    """records in a box in front of, beside and behind a camera at the origin looking along +z"""
    p = random_cloud(rng, n, nan=nan)
    p["x"] = np.where(np.isfinite(p["x"]), rng.uniform(-half, half, n).astype(F), p["x"])
    p["y"] = rng.uniform(-half, half, n).astype(F)
    p["z"] = np.where(np.isfinite(p["z"]), rng.uniform(-0.5, depth[1], n).astype(F), p["z"])
    return p


@pytest.mark.parametrize("s", [0, 2])
def test_mirror_equals_the_per_pixel_loop(s):
    rng = np.random.default_rng(10 + s)
    rows, cols = 12, 16
    p = cloud_around(rng, 300)
    p["z"][:40] = p["z"][40:80]; p["x"][:40] = p["x"][40:80]; p["y"][:40] = p["y"][40:80]     # ties in Z: the smaller index wins
    R, t = rotation(rng, 0.2), rng.uniform(-0.1, 0.1, 3)
    got = RM.render_numpy(p, R[None], t[None], K_TINY, rows, cols, s, 0.3, 2.5)
    index, depth = RM.render_bruteforce(p, R, t, K_TINY, rows, cols, s, 0.3, 2.5)
    gi = got["index"][0].astype(np.int64)
    gi[got["index"][0] == RM.EMPTY] = -1
    assert np.array_equal(gi, index)
    assert np.array_equal(got["depth"][0].view(np.uint32), RM.one_nan(depth).view(np.uint32))
    hit = index >= 0
    assert 20 < hit.sum() < rows * cols or s == 2
    w = p[np.where(hit, index, 0)]
    assert np.array_equal(got["colour"][0][hit], np.stack([w["r"], w["g"], w["b"]], -1)[hit]) and not got["colour"][0][~hit].any()
    assert (got["normal"][0].view(np.uint32)[:, ~hit] == RM.NAN_BITS).all()
    m = RM.pose_cw(R, t)
    for a in range(3):                                    # the normal: R_CW n in float32, one rounding per operation, NaN as one pattern
        with np.errstate(invalid="ignore"):
            e = RM.one_nan(((m[3 * a] * w["nx"] + m[3 * a + 1] * w["ny"]) + m[3 * a + 2] * w["nz"]).astype(F))
        assert np.array_equal(got["normal"][0][a].view(np.uint32)[hit], e.view(np.uint32)[hit])
    assert np.isnan(got["normal"][0][:, hit]).any()       # random_cloud's NaN normals take part and come out as NaN_BITS


def test_mirror_by_hand():
    """identity pose, K = (2, 2, 1.5, 1.5), 4 x 4: (0, 0, 1) -> u = v = 1.5, pu = pv = floor(2.0) = 2; (0.25, 0, 1) -> u = 2.0, pu = 2 too and
    farther records lose; Z = z_min and z_max stay, one ulp outside go"""
    p = np.zeros(6, CL.POINT_DTYPE)
    p["x"] = [0, 0.25, 0, -0.75, -0.75, -0.75]
    p["y"] = [0, 0, 0, -0.75, -0.75, -0.75]
    p["z"] = [1, 1, 0.5, 2, np.nextafter(F(2), F(3)), np.nextafter(F(0.5), F(0))]
    p["r"] = [10, 20, 30, 40, 50, 60]
    out = RM.render_numpy(p, np.eye(3)[None], np.zeros((1, 3)), (2, 2, 1.5, 1.5), 4, 4, 0, 0.5, 2.0)
    idx = out["index"][0]
    assert idx[2, 2] == 2 and out["depth"][0][2, 2] == 0.5 and out["colour"][0][2, 2, 0] == 30        # the nearest of 0, 1, 2
    assert idx[1, 1] == 3 and out["depth"][0][1, 1] == 2.0      # (-0.75 / 2) * 2 + 1.5 = 0.75 -> floor(1.25) = 1; Z = z_max stays
    assert (idx != RM.EMPTY).sum() == 2                  # 4 (beyond z_max) and 5 (before z_min) are gated
    out = RM.render_numpy(p[:2], np.eye(3)[None], np.zeros((1, 3)), (2, 2, 1.5, 1.5), 4, 4, 1, 0.5, 2.0)
    assert (out["index"][0][1:4, 1:4] == 0).all() and (out["index"][0][0] == RM.EMPTY).all()         # equal Z: the smaller index


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_pose_as_twelve_floats_equals_the_library():
    rng = np.random.default_rng(3)
    for k in range(20):
        R, t = rotation(rng, 3.0), rng.uniform(-5, 5, 3) * (10.0 ** rng.integers(-3, 3))
        assert np.array_equal(RD.pose_cw(R, t).view(np.uint32), RM.pose_cw(R, t).view(np.uint32))
    m = RM.pose_cw(np.eye(3), [1, 2, 3])
    assert m.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, -1, -2, -3]
    L = _lib_handle()
    out = (ctypes.c_float * 12)()
    assert L.rgbid_render_pose_cw(None, out) == -1 and L.rgbid_render_pose_cw(ctypes.byref(RD.Pose()), None) == -1


def test_python_argument_validation_needs_no_device():
    assert RD.image_size(480, 640, 16, 480 * 640 * 16) == (480, 640) and RD.splat_arg(np.int64(4)) == 4 and RD.splat_arg(0) == 0
    assert RD.depth_range(0.05, 20) == (float(F(0.05)), 20.0) and RD.depth_range(1, 1) == (1.0, 1.0)
    assert RD.intrinsics((525, 525.5, 319.5, 239.5)) == [525.0, 525.5, 319.5, 239.5]
    R, t = RD.poses(np.eye(3), [0, 0, 1])
    assert R.shape == (1, 3, 3) and t.shape == (1, 3)
    assert RD.outputs_arg("index") == ("index",) and RD.outputs_arg(["depth", "normal"]) == ("depth", "normal")
    for rows, cols, views, cap in ((0, 4, 1, None), (4, 0, 1, None), (-1, 4, 1, None), (4, 4, 0, None), (4, 4, 2, 31), ((1 << 20) + 1, 1, 1, None),
                                   (4.0, 4, 1, None), (True, 4, 1, None)):
        with pytest.raises(ValueError):
            RD.image_size(rows, cols, views, cap)
    for s in (-1, 5, 1.0, "1", None, True):
        with pytest.raises(ValueError):
            RD.splat_arg(s)
    for lo, hi in ((0, 1), (-1, 1), (2, 1), (NAN, 1), (1, NAN), (1, INF), (INF, INF), (1e-50, 1), ("a", 1), (None, 2)):
        with pytest.raises(ValueError):
            RD.depth_range(lo, hi)
    for K in ((0, 1, 1, 1), (1, 0, 1, 1), (NAN, 1, 1, 1), (1, 1, INF, 1), (1, 1, 1), (1, 1, 1, 1e40), "K"):
        with pytest.raises(ValueError):
            RD.intrinsics(K)
    bad = np.eye(3); bad[1, 2] = NAN
    for R, t in ((bad, [0, 0, 0]), (np.eye(3), [0, INF, 0]), (np.eye(3), [0, 1e300, 0]), (np.eye(3) * 1e39, [0, 0, 0]), (np.zeros((2, 3, 3)), np.zeros((3, 3))),
                 (np.zeros((0, 3, 3)), np.zeros((0, 3))), (np.eye(4), [0, 0, 0])):
        with pytest.raises(ValueError):
            RD.poses(R, t)
    for o in ((), ("depth", "color"), "rgb"):
        with pytest.raises(ValueError):
            RD.outputs_arg(o)

    class NoDevice:                                      # render_views validates before it creates anything
        shape = (0, 32)
    good = dict(R=np.eye(3), t=np.zeros(3), K=(10, 10, 4, 4), rows=8, cols=8)
    for change in (dict(rows=0), dict(splat=5), dict(z_min=0.0), dict(z_min=3.0, z_max=2.0), dict(K=(0, 10, 4, 4)), dict(t=[NAN, 0, 0]),
                   dict(outputs=("depth", "x"))):
        with pytest.raises(ValueError):
            RD.render_views(None, NoDevice(), **dict(good, **change))
    assert RD.rank_value([1.0, 2.0, 3.0, 4.0], 5) == 2.0 and RD.rank_value(np.arange(1, 11), 9) == 9 and RD.rank_value([7.0], 9) == 7.0
    assert np.isnan(RD.rank_value([], 5))
    assert RD.depth_png(np.array([[NAN, 1.0, 0.0002, 20.0]], F)).tolist() == [[0, 5000, 1, 65535]]


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_render.c"
    src.write_text('#include "rgbid_render.h"\n'
                   "typedef char pose_is_12_doubles[sizeof(rgbid_render_pose) == 96 ? 1 : -1];\n"
                   "typedef char empty_is_no_index[RGBID_RENDER_EMPTY > RGBID_RENDER_MAX_POINTS - 1 ? 1 : -1];\n"
                   "int use(rgbid_render* r, const rgbid_cloud_point* p, const rgbid_render_pose* v, uint32_t* i, float* d, uint8_t* c) {\n"
                   "  const float K[4] = {525.f, 525.f, 319.5f, 239.5f}; float ms[3]; unsigned long long st[3];\n"
                   "  return rgbid_render_views(r, p, 0, RGBID_RENDER_VIEW_CHUNK, v, K, 480, 640, RGBID_RENDER_MAX_SPLAT, 0.05f, 20.f, i, d, c, d)\n"
                   "       + rgbid_render_timing(r, 1, ms) + rgbid_render_stats(r, 0, st); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_render.h")).read()
    assert int(re.search(r"RGBID_RENDER_MAX_SPLAT\s+(\d+)", txt).group(1)) == RD.MAX_SPLAT
    assert int(re.search(r"RGBID_RENDER_MAX_POINTS\s+(\d+)ull", txt).group(1)) == RD.MAX_POINTS
    assert int(re.search(r"RGBID_RENDER_MAX_DIM\s+(\d+)", txt).group(1)) == RD.MAX_DIM
    assert int(re.search(r"RGBID_RENDER_VIEW_CHUNK\s+(\d+)", txt).group(1)) == RD.VIEW_CHUNK
    assert int(re.search(r"RGBID_RENDER_EMPTY\s+(0x[0-9A-Fa-f]+)u", txt).group(1), 16) == RD.EMPTY == int(RM.EMPTY)
    assert int(re.search(r"RGBID_RENDER_NAN_BITS\s+(0x[0-9A-Fa-f]+)u", txt).group(1), 16) == RD.NAN_BITS == int(RM.NAN_BITS)


def test_library_exports_render_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_render.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_render_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(RD.EXPORTS), set(declared) ^ set(RD.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    """argument checks come before the library touches the runtime: a null renderer, a null context, capacities of 0 or past the bounds"""
    L = _lib_handle()
    L.rgbid_render_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_ulonglong]
    L.rgbid_render_views.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float] + [ctypes.c_void_p] * 4
    L.rgbid_render_timing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.rgbid_render_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    h = ctypes.c_void_p()
    assert L.rgbid_render_create(ctypes.byref(h), None, 10, 10) == -1 and not h.value
    assert L.rgbid_render_create(None, None, 10, 10) == -1
    pose = RD.Pose((ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_double * 3)(0, 0, 0))
    k = (ctypes.c_float * 4)(10, 10, 4, 4)
    assert L.rgbid_render_views(None, None, 0, 1, ctypes.byref(pose), k, 8, 8, 1, 0.05, 20.0, None, None, None, None) == -1
    assert L.rgbid_render_timing(None, 0, None) == -1 and L.rgbid_render_stats(None, 0, None) == -1
    assert L.rgbid_render_destroy(None) == 0


def test_cli_refuses_render_without_cloud(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    for bad, word in ((["--render", str(tmp_path / "views")], "--render needs --cloud"),
                      (["--render-check"], "--render-check needs --cloud"),
                      (["--cloud", str(tmp_path / "m.ply"), "--render-splat", "1"], "--render-splat needs --render"),
                      (["--cloud", str(tmp_path / "m.ply"), "--render", str(tmp_path / "views"), "--render-splat", "5"], "splat must lie in")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "views").exists() and not (tmp_path / "m.ply").exists()
