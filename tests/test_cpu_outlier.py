"""CPU checks of the radius outlier filter (include/rgbid_outlier.h, rgbid.outlier): the numpy restatements the GPU tests compare the
kernels against (tests/outlier_mirror.py) -- the grid mirror against brute force, a hand-computed line, non-finite records, the clamp;
the Python argument checks; the header as C99; the library's exports; refusals that need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import cloud as CL
from rgbid import outlier as OL
from tests.outlier_mirror import radius_counts_bruteforce, radius_counts_grid, radius_filter_numpy
from tests.test_cpu_cloud import records_equal
from tests.test_cpu_voxel import random_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32


def xyz_cloud(x, y=None, z=None):
    """positions -> POINT_DTYPE records (zero normals and colours, pixel = the row number)"""
    x = np.asarray(x, np.float32)
    p = np.zeros(len(x), CL.POINT_DTYPE)
    p["x"] = x
    p["y"] = 0 if y is None else np.asarray(y, np.float32)
    p["z"] = 0 if z is None else np.asarray(z, np.float32)
    p["pixel"] = np.arange(len(x))
    return p


def clustered_cloud(rng, n, clusters=12, spread=0.01):
    c = rng.uniform(-0.3, 0.3, (clusters, 3))
    q = c[rng.integers(0, clusters, n)] + rng.normal(scale=spread, size=(n, 3))
    p = random_cloud(rng, n, nan=0.02)
    for a, f in enumerate("xyz"):
        p[f] = np.where(np.isfinite(p[f]), q[:, a].astype(np.float32), p[f])
    return p


def duplicated_cloud(rng, n):
    p = random_cloud(rng, n, spread=0.03, nan=0.02)
    src = rng.integers(0, n // 4, n)                    # every record is a copy of one of the first n / 4
    for f in "xyz":
        p[f] = p[f][src]
    return p


def test_line_at_r_and_one_ulp_either_side():
    """r = 1, r2 = 1.  e = -(1 + 2^-23), a = -1, b = 0, c = 1 - 2^-24, d = 2 - 2^-23; every difference below is exact in float32.
    a-b: dx = 1, d2 = 1 <= 1: neighbours.  b-c and c-d: dx = 1 - 2^-24 (r less one ulp), dx dx = 1 - 2^-23 + 2^-48 -> 1 - 2^-23: neighbours.
    e-b: dx = 1 + 2^-23 (r plus one ulp), dx dx = 1 + 2^-22 + 2^-46 -> 1 + 2^-22 > 1: not.  e-a: dx = 2^-23: neighbours.  The rest are ~2 apart."""
    x = [-(1 + 2.0 ** -23), -1.0, 0.0, 1 - 2.0 ** -24, 2 - 2.0 ** -23]
    assert [float(F(v)) for v in x] == x and x[3] == float(np.nextafter(F(1), F(0))) and -x[0] == float(np.nextafter(F(1), F(2)))
    p = xyz_cloud(x)
    for axes in ("xyz", "yzx", "zxy"):                   # the same line along each axis
        q = xyz_cloud(p[axes[0]], p[axes[1]], p[axes[2]])
        assert radius_counts_bruteforce(q, 1.0, 10).tolist() == [1, 2, 2, 2, 1]
        assert radius_counts_grid(q, 1.0, 10).tolist() == [1, 2, 2, 2, 1]
    counts, mask, kept = radius_filter_numpy(p, 1.0, 2)
    assert counts.tolist() == [1, 2, 2, 2, 1] and mask.tolist() == [False, True, True, True, False] and kept["pixel"].tolist() == [1, 2, 3]
    assert radius_counts_bruteforce(p, 1.0, 1).tolist() == [1] * 5                       # the clamp
    assert radius_counts_bruteforce(p, np.nextafter(F(1), F(0)), 10).tolist() == [1, 1, 1, 2, 1]   # r2 = 1 - 2^-23: a-b goes, b-c and c-d stay


@pytest.mark.parametrize("seed", range(3))
def test_grid_mirror_equals_bruteforce(seed):
    rng = np.random.default_rng(seed)
    n = (1500, 3000, 4096)[seed]
    for name, p in (("random", random_cloud(rng, n)), ("clustered", clustered_cloud(rng, n)), ("duplicated", duplicated_cloud(rng, n))):
        for r, cap in ((0.01, 1 << 31), (0.004, 3), (0.05, 16)):
            b = radius_counts_bruteforce(p, r, cap)
            g = radius_counts_grid(p, r, cap, chunk=50_000)                             # several chunks per offset
            np.testing.assert_array_equal(b, g, err_msg=f"{name} r={r} cap={cap}")
            assert b.max() <= cap and (b[~np.isfinite(p["x"])] == 0).all()
    d = duplicated_cloud(rng, 400)
    fin = np.isfinite(d["x"]) & np.isfinite(d["y"]) & np.isfinite(d["z"])
    c = radius_counts_bruteforce(d, 2.0 ** -60, 1 << 31)                                 # only exact duplicates are within 2^-60
    key = np.stack([d[f][fin] for f in "xyz"], 1)
    _, inv, num = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    np.testing.assert_array_equal(c[fin], num[inv.reshape(-1)] - 1)


def test_non_finite_records_take_no_part():
    p = xyz_cloud([0.0, 0.001, NAN, 0.002, INF, 0.0015], [0, 0, 0, NAN, 0, 0], [0, 0, 0, 0, 0, -INF])
    p["nx"][1] = NAN                                     # a NaN normal does not exclude a record
    counts, mask, kept = radius_filter_numpy(p, 0.01, 0)
    assert counts.tolist() == [1, 1, 0, 0, 0, 0] and mask.tolist() == [True, True, False, False, False, False]
    assert records_equal(kept, p[:2])[0]
    counts, mask, kept = radius_filter_numpy(p, 0.01, 1, cap=5)
    assert mask.tolist() == [True, True, False, False, False, False]
    counts, mask, kept = radius_filter_numpy(p, 0.01, 2, cap=5)
    assert not mask.any() and len(kept) == 0
    q = p.copy(); q["x"] = NAN
    counts, mask, kept = radius_filter_numpy(q, 0.01, 0)
    assert not counts.any() and not mask.any()
    assert len(radius_filter_numpy(np.zeros(0, CL.POINT_DTYPE), 0.01, 1)[2]) == 0


def test_cap_clamps_and_min_neighbours_zero_keeps_the_finite():
    rng = np.random.default_rng(5)
    p = random_cloud(rng, 2000, spread=0.02)
    full = radius_counts_bruteforce(p, 0.01, 1 << 31)
    assert full.max() > 8
    for cap in (1, 2, 8):
        np.testing.assert_array_equal(radius_counts_bruteforce(p, 0.01, cap), np.minimum(full, cap))
        np.testing.assert_array_equal(radius_counts_grid(p, 0.01, cap), np.minimum(full, cap))
    fin = np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])
    counts, mask, kept = radius_filter_numpy(p, 0.01, 0)
    np.testing.assert_array_equal(mask, fin)
    assert counts.max() == 1 and records_equal(kept, p[fin])[0]                         # the default cap is max(min_neighbours, 1)
    counts, mask, kept = radius_filter_numpy(p, 0.01, 4)
    np.testing.assert_array_equal(counts, np.minimum(full, 4))
    np.testing.assert_array_equal(mask, fin & (full >= 4))


def test_python_argument_validation_needs_no_device():
    assert OL.radius32(0.02) == float(F(0.02)) and OL.neighbour_args(4) == (4, 4) and OL.neighbour_args(0) == (0, 1)
    assert OL.neighbour_args(2, 7) == (2, 7) and OL.neighbour_args(np.int64(3), 1 << 31) == (3, 1 << 31)
    assert OL.cell_size(0.02) == F(0.02) * F(1.0625)
    for bad in (0, -0.02, NAN, INF, -INF, 1e-30, 1e30, "r", None):
        with pytest.raises(ValueError):
            OL.radius32(bad)
    for m, cap in ((-1, None), (2, 1), (0, 0), (1, 1 << 32), (1.5, None), (1, 2.0), (True, None)):
        with pytest.raises(ValueError):
            OL.neighbour_args(m, cap)

    class NoDevice:                                      # radius_filter validates before it creates anything
        shape = (0, 32)
        device = "cpu"
    for args in ((0.0, 1), (NAN, 1), (0.02, 3, 2), (0.02, -1)):
        with pytest.raises(ValueError):
            OL.radius_filter(None, NoDevice(), *args)
    import torch
    out, cnt, plan = OL.radius_filter(None, torch.empty((0, 32), dtype=torch.uint8), 0.02, 4, return_counts=True, return_plan=True)
    assert out.shape == (0, 32) and cnt.shape == (0,) and (plan.kept, plan.n, plan.finite, plan.cells) == (0, 0, 0, 0)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_outlier.c"
    src.write_text('#include "rgbid_outlier.h"\n'
                   "typedef char bound_is_2_18[RGBID_OUTLIER_MAX_CELL == (1 << 18) ? 1 : -1];\n"
                   "int use(rgbid_outlier* o, const rgbid_cloud_point* p, uint32_t* c) { unsigned long long s[3], k;\n"
                   "  return rgbid_outlier_plan(o, p, 0, 0.02f * RGBID_OUTLIER_CELL_FACTOR, 4u, 4u, s, &k) + rgbid_outlier_counts(o, c); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_outlier.h")).read()
    assert float(re.search(r"RGBID_OUTLIER_MIN_RADIUS\s+(\S+?)f\b", txt).group(1)) == OL.MIN_RADIUS
    assert float(re.search(r"RGBID_OUTLIER_MAX_RADIUS\s+(\S+?)f\b", txt).group(1)) == OL.MAX_RADIUS
    assert float(re.search(r"RGBID_OUTLIER_CELL_FACTOR\s+(\S+?)f\b", txt).group(1)) == float(OL.CELL_FACTOR)
    assert int(re.search(r"RGBID_OUTLIER_MAX_CELL\s+(\d+)", txt).group(1)) == OL.MAX_CELL


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_outlier_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_outlier.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_outlier_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(OL.EXPORTS), set(declared) ^ set(OL.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    """argument checks come before the library touches the runtime: a null filter, a null context, a capacity past 2^31"""
    L = _lib_handle()
    L.rgbid_outlier_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_uint, ctypes.c_uint,
                                     ctypes.c_void_p, ctypes.c_void_p]
    L.rgbid_outlier_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong]
    L.rgbid_outlier_emit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong]
    L.rgbid_outlier_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.rgbid_outlier_timing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    k = ctypes.c_ulonglong(7)
    for radius in (0.02, 0.0, NAN):
        assert L.rgbid_outlier_plan(None, None, 0, radius, 1, 1, None, ctypes.byref(k)) == -1
    h = ctypes.c_void_p()
    assert L.rgbid_outlier_create(ctypes.byref(h), None, 10) == -1 and not h.value
    assert L.rgbid_outlier_create(None, None, 10) == -1
    assert L.rgbid_outlier_emit(None, None, 0) == -1
    assert L.rgbid_outlier_counts(None, None) == -1
    assert L.rgbid_outlier_timing(None, 0, None) == -1
    assert L.rgbid_outlier_destroy(None) == 0
