"""CPU checks of the voxel-grid filter (include/rgbid_voxel.h, rgbid.voxel): the numpy restatement the GPU tests compare the kernels
against (tests/voxel_mirror.py), on a hand-computed cloud and against an independent loop-and-dict restatement on random clouds; the
header as C99; the library's exports; refusals that need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import cloud as CL
from rgbid import voxel as VX
from tests.test_cpu_cloud import records_equal
from tests.voxel_mirror import Refused, voxel_loops, voxel_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def cloud(rows):
    """[(x, y, z, nx, ny, nz, r, g, b, flags)] -> POINT_DTYPE records (pixel = the row number)"""
    p = np.zeros(len(rows), CL.POINT_DTYPE)
    for i, r in enumerate(rows):
        for f, v in zip(("x", "y", "z", "nx", "ny", "nz", "r", "g", "b", "flags"), r):
            p[f][i] = v
        p["pixel"][i] = i
    return p


# leaf (0.5, 0.5, 0.25): inv = (2, 2, 4) exactly; every coordinate below is exact in float32, so the cells can be read off by hand
KAT_LEAF = (0.5, 0.5, 0.25)
KAT = [
    (-0.125, 0.25, 0.125, 0.0, 0.0, 1.0, 254, 10, 0, 1),     # 0: floor(-0.25) = -1, floor(0.5) = 0, floor(0.5) = 0
    (-0.375, 0.375, 0.0625, NAN, 0.0, 0.0, 255, 11, 1, 0),   # 1: same cell; NaN normal x: its normal is left out
    (0.5, 0.0, 0.0, NAN, NAN, NAN, 7, 7, 7, 1),              # 2: x * inv = 1.0 exactly: the next cell
    (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1, 2, 3, 0),              # 3
    (NAN, 0.0, 0.0, 1.0, 0.0, 0.0, 9, 9, 9, 1),              # 4: NaN position: dropped
    (INF, 1.0, 1.0, 1.0, 0.0, 0.0, 9, 9, 9, 1),              # 5: infinite position: dropped
    (0.25, 0.375, 0.1875, 0.0, 1.0, 0.0, 2, 3, 4, 0),        # 6: cell of 3 (0.75 floors to 0 on every axis)
    (-0.5, 1.0, 0.5, 0.0, 0.0, 0.0, 100, 200, 50, 2),        # 7: a cell of its own; zero normal sum -> NaN; flags bit 1 is not carried
    (0.0, 0.0, -0.0, 1.0, 0.0, 0.0, 3, 4, 5, 0),             # 8: -0: cell of 3
]


def test_voxel_numpy_kat():
    got, plan = voxel_numpy(cloud(KAT), KAT_LEAF, return_plan=True)
    assert plan["min_b"] == [-1, 0, 0] and plan["div_b"] == [3, 3, 3]
    assert (plan["finite"], plan["runs"], plan["kept"]) == (7, 4, 4)
    # keys: points 0, 1 -> (0, 0, 0) = 0; 3, 6, 8 -> (1, 0, 0) = 1; 2 -> (2, 0, 0) = 2; 7 -> (0, 2, 2) = 2 * 3 + 2 * 9 = 24
    s5 = np.float32(1 / np.sqrt(5.0))
    expect = [  # centroid, normal, count, colour, flags
        ((-0.25, 0.3125, 0.09375), (0.0, 0.0, 1.0), 2, (254, 10, 0), 1),        # colour: 509 // 2 = 254, 21 // 2 = 10, 1 // 2 = 0
        ((np.float32(0.25 / 3), 0.125, 0.0625), (2 * s5, s5, 0.0), 3, (2, 3, 4), 0),   # normal sum (2, 1, 0) / sqrt(5)
        ((0.5, 0.0, 0.0), (NAN, NAN, NAN), 1, (7, 7, 7), 1),                     # no finite normal
        ((-0.5, 1.0, 0.5), (NAN, NAN, NAN), 1, (100, 200, 50), 0),               # normal sum 0
    ]
    assert len(got) == 4
    for g, (X, n, c, rgb, fl) in zip(got, expect):
        np.testing.assert_array_equal([g["x"], g["y"], g["z"]], np.float32(X))
        np.testing.assert_array_equal([g["nx"], g["ny"], g["nz"]], np.float32(n))
        assert (g["count"], (g["r"], g["g"], g["b"]), g["flags"]) == (c, rgb, fl)
    ok, first = records_equal(got, voxel_loops(cloud(KAT), KAT_LEAF))
    assert ok, first
    two, plan = voxel_numpy(cloud(KAT), KAT_LEAF, min_points=2, return_plan=True)
    assert (plan["runs"], plan["kept"]) == (4, 2) and two["count"].tolist() == [2, 3]
    assert records_equal(two, got[:2])[0]
    assert len(voxel_numpy(cloud(KAT), KAT_LEAF, min_points=4)) == 0


def test_voxel_numpy_isotropic_leaf_and_truncation():
    """one scalar leaf for all axes; the centroid is (sum in double) / n rounded once; colour 254, 255 -> 254"""
    pts = cloud([(0.001, 0.002, 0.003, 0, 0, 1, 254, 0, 255, 0), (0.004, 0.005, 0.006, 0, 0, 1, 255, 1, 255, 0),
                 (0.011, 0.0, 0.0, 0, 0, 1, 0, 0, 0, 0)])
    got = voxel_numpy(pts, 0.01)
    assert got["count"].tolist() == [2, 1]
    assert got["x"][0] == np.float32((np.float64(np.float32(0.001)) + np.float64(np.float32(0.004))) / 2)
    assert (got["r"][0], got["g"][0], got["b"][0]) == (254, 0, 255)


def test_voxel_numpy_empty_and_refusals():
    assert len(voxel_numpy(np.zeros(0, CL.POINT_DTYPE), 0.01)) == 0
    assert len(voxel_numpy(cloud([(NAN, 0, 0, 0, 0, 0, 0, 0, 0, 0)]), 0.01)) == 0
    for leaf in (0.0, -0.01, NAN, INF, (0.01, 0.01, 0.0), (0.01, 0.01)):
        with pytest.raises(ValueError):
            voxel_numpy(cloud(KAT), leaf)
    with pytest.raises(Refused):                                   # floor(3e9 / 1) is outside int32
        voxel_numpy(cloud([(3e9, 0, 0, 0, 0, 0, 0, 0, 0, 0)]), 1.0)
    with pytest.raises(Refused):                                   # 2^21 x 2^21 x 2^21 cells = 2^63
        voxel_numpy(cloud([(0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (2.0 ** 21 - 1, 2.0 ** 21 - 1, 2.0 ** 21 - 1, 0, 0, 0, 0, 0, 0, 0)]), 1.0)
    _, plan = voxel_numpy(cloud([(0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (2.0 ** 20, 2.0 ** 20, 2.0 ** 20, 0, 0, 0, 0, 0, 0, 0)]), 1.0, return_plan=True)
    assert plan["div_b"] == [2 ** 20 + 1] * 3 and plan["key_bits"] == 61  # past 2^32 cells: the 64-bit key path


def random_cloud(rng, n, spread=0.05, nan=0.05):
    p = np.zeros(n, CL.POINT_DTYPE)
    for c in "xyz":
        p[c] = rng.normal(scale=spread, size=n).astype(np.float32)
    for c in ("nx", "ny", "nz"):
        p[c] = rng.normal(size=n).astype(np.float32)
    p["x"][rng.random(n) < nan] = np.nan
    p["z"][rng.random(n) < nan / 2] = np.inf
    p["ny"][rng.random(n) < 0.1] = np.nan
    for c in "rgb":
        p[c] = rng.integers(0, 256, n)
    p["flags"] = rng.integers(0, 2, n)
    p["pixel"] = np.arange(n)
    return p


@pytest.mark.parametrize("seed", range(4))
def test_voxel_numpy_against_loops(seed):
    rng = np.random.default_rng(seed)
    p = random_cloud(rng, 700 + 300 * seed)
    for leaf, minp in ((0.01, 0), (0.02, 3), ((0.01, 0.03, 0.005), 0), (1.0, 0), (0.001, 2)):
        ok, first = records_equal(voxel_numpy(p, leaf, minp), voxel_loops(p, leaf, minp))
        assert ok, (leaf, minp, first)


def test_leaf_normalisation():
    assert VX.leaf3(0.01) == [float(np.float32(0.01))] * 3
    assert VX.leaf3((1, 2, 3)) == [1.0, 2.0, 3.0]
    for bad in (0, -1, NAN, INF, (1, 2), (1, 2, 0)):
        with pytest.raises(ValueError):
            VX.leaf3(bad)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_voxel.c"
    src.write_text('#include "rgbid_voxel.h"\n'
                   "#include <stddef.h>\n"
                   "typedef char voxel_is_32_bytes[sizeof(rgbid_voxel_point) == 32 ? 1 : -1];\n"
                   "typedef char count_is_pixel[offsetof(rgbid_voxel_point, count) == offsetof(rgbid_cloud_point, pixel) ? 1 : -1];\n"
                   "int use(rgbid_voxel* v, const rgbid_cloud_point* p) { float l[3] = {0.01f, 0.01f, 0.01f}; long long g[6];\n"
                   "  unsigned long long s[3], n; return rgbid_voxel_plan(v, p, 0, l, 0u, g, s, &n); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_voxel_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_voxel.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_voxel_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(VX.EXPORTS), set(declared) ^ set(VX.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    """argument checks come before the library touches the runtime: a null filter, a null context, a capacity past 2^31"""
    L = _lib_handle()
    L.rgbid_voxel_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p]
    L.rgbid_voxel_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong]
    L.rgbid_voxel_emit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong]
    n = ctypes.c_ulonglong(7)
    for leaf in ((0.01, 0.01, 0.01), (0.0, 0.01, 0.01), (NAN, 1.0, 1.0)):
        lf = (ctypes.c_float * 3)(*leaf)
        assert L.rgbid_voxel_plan(None, None, 0, lf, 0, None, None, ctypes.byref(n)) == -1
    h = ctypes.c_void_p()
    assert L.rgbid_voxel_create(ctypes.byref(h), None, 10) == -1 and not h.value
    assert L.rgbid_voxel_create(None, None, 10) == -1
    assert L.rgbid_voxel_emit(None, None, 0) == -1
    assert L.rgbid_voxel_destroy(None) == 0
