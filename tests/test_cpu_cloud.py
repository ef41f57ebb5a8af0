"""CPU checks of the keyframe point cloud (include/rgbid_cloud.h, rgbid.cloud): the float64 restatement of the reference's
KeyframeManager::computeAlignedPointCloud (src/keyframe_manager.cpp:438-528) that the GPU tests compare the kernels against, checked
here on a hand-computed 3 x 4 keyframe; the library's Kinv; the PLY layout; the header as C99; the library's exports."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import cloud as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kinv_numpy(K):
    """Eigen's compute_inverse<3x3> of K = [fx 0 cx; 0 fy cy; 0 0 1] (float K widened to double): Kinv(i, j) = cofactor(j, i) / det"""
    fx, fy, cx, cy = [np.float64(np.float32(v)) for v in K]
    z, o = np.float64(0.0), np.float64(1.0)
    m = [[fx, z, cx], [z, fy, cy], [z, z, o]]

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]

    det = (cof(0, 0) * m[0][0] + cof(1, 0) * m[1][0]) + cof(2, 0) * m[2][0]
    invdet = o / det
    return np.array([[cof(j, i) * invdet for j in range(3)] for i in range(3)], np.float64)


def split_block(block, rows, cols):
    """packed export block (u8 [20 N]) -> overlap mask u8 [N], colours u8 [N, 3], inverse depth f32 [N], normals f32 [3, N]"""
    N = rows * cols
    b = np.ascontiguousarray(block, np.uint8).reshape(-1)
    assert b.size == 20 * N
    return b[:N], b[N:4 * N].reshape(N, 3), b[4 * N:8 * N].view("<f4"), b[8 * N:20 * N].view("<f4").reshape(3, N)


def make_block(mask, colors, iD, normals):
    return np.concatenate([np.asarray(mask, np.uint8).reshape(-1), np.asarray(colors, np.uint8).reshape(-1),
                           np.asarray(iD, "<f4").reshape(-1).view(np.uint8), np.asarray(normals, "<f4").reshape(-1).view(np.uint8)])


def cloud_numpy(block, rows, cols, K, R, t, mode):
    """The reference's loop in float64 numpy, in the evaluation order the kernel fixes: d = 1.f / iD (float); a pixel is kept when d and
    the normal's x are not NaN (and, mode "novel", its overlap mask is 0); Xcam_i = ((d Kinv_i0 x + d Kinv_i1 y) + d Kinv_i2 1.0),
    Xworld_i = ((R_i0 X0 + R_i1 X1) + R_i2 X2) + t_i, nworld_i = (R_i0 n0 + R_i1 n1) + R_i2 n2, rounded to float.  -> POINT_DTYPE records"""
    mask, colors, iD, nrm = split_block(block, rows, cols)
    with np.errstate(all="ignore"):
        d = np.float32(1.0) / iD
        keep = ~np.isnan(d) & ~np.isnan(nrm[0])
        if mode in ("novel", CL.NOVEL_ONLY):
            keep &= mask == 0
        p = np.nonzero(keep)[0]
        x = (p % cols).astype(np.float64); y = (p // cols).astype(np.float64); one = np.ones_like(x)
        dd = d[p].astype(np.float64)
        Ki = kinv_numpy(K); R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
        Xc = [((dd * Ki[i, 0]) * x + (dd * Ki[i, 1]) * y) + (dd * Ki[i, 2]) * one for i in range(3)]
        Xw = [((R[i, 0] * Xc[0] + R[i, 1] * Xc[1]) + R[i, 2] * Xc[2]) + t[i] for i in range(3)]
        n = [nrm[c][p].astype(np.float64) for c in range(3)]
        nw = [(R[i, 0] * n[0] + R[i, 1] * n[1]) + R[i, 2] * n[2] for i in range(3)]
    out = np.zeros(len(p), CL.POINT_DTYPE)
    for i, c in enumerate("xyz"):
        out[c] = Xw[i].astype(np.float32)
        out["n" + c] = nw[i].astype(np.float32)
    out["pixel"] = p
    out["r"], out["g"], out["b"] = colors[p, 0], colors[p, 1], colors[p, 2]
    out["flags"] = np.where(mask[p] == 0, CL.FLAG_NOVEL, 0)
    return out


def records_equal(a, b):
    """all 32 bytes of every record equal, except that a NaN float equals any NaN (the payload and sign of a NaN that an arithmetic
    operation produces differ between the host's and the device's floating-point units); -> (ok, first differing record)"""
    a = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 8).copy(); b = np.ascontiguousarray(b).view(np.uint32).reshape(-1, 8).copy()
    if a.shape != b.shape:
        return False, None
    for m in (a, b):
        f = m[:, :6]
        f[(f & 0x7f800000 == 0x7f800000) & (f & 0x007fffff != 0)] = 0x7fc00000
    bad = np.nonzero((a != b).any(1))[0]
    return bad.size == 0, (int(bad[0]) if bad.size else None)


# ---- the hand-computed 3 x 4 keyframe -------------------------------------------------------------------------------------------
KAT_K = (2.0, 4.0, 1.0, 0.5)             # Kinv = [[0.5, 0, -0.5], [0, 0.25, -0.125], [0, 0, 1]] exactly
KAT_T = (1.0, 2.0, 3.0)
NAN = float("nan")
DENORM = float(np.ldexp(np.float32(1), -127))   # a float32 denormal whose reciprocal 2^127 is finite


def kat_block():
    rows, cols = 3, 4
    iD = [[NAN, 0.0, -0.0, -2.0],
          [DENORM, float("inf"), 1.0, 1.0],
          [1.0, 0.5, 0.25, 2.0]]
    mask = [[0, 0, 1, 0], [1, 0, 0, 1], [1, 0, 1, 0]]
    n = np.zeros((3, rows, cols), np.float32)
    n[0], n[1], n[2] = 0.6, 0.0, -0.8
    n[0, 1, 2] = NAN                                # pixel (2, 1): normal x NaN -> skipped
    n[1, 1, 3] = NAN                                # pixel (3, 1): only normal y NaN -> kept
    col = np.array([[10 * p, 10 * p + 1, 10 * p + 2] for p in range(rows * cols)], np.uint8)
    return make_block(mask, col, np.array(iD, np.float32), n), rows, cols


def test_cloud_numpy_kat():
    block, rows, cols = kat_block()
    got = cloud_numpy(block, rows, cols, KAT_K, np.eye(3), KAT_T, "all")
    nan3 = (NAN, NAN, NAN)
    n = (0.6, 0.0, -0.8)   # R = I: nworld = ncam (0 * n is 0 for finite n)
    big = (-2.0 ** 126, 2.0 ** 124, 2.0 ** 127)     # d = 2^127: Xcam = (-2^126, 2^124, 2^127); + t is lost in the rounding to float
    expect = [  # pixel, Xworld, nworld, novel
        (1, nan3, n, 1),                        # iD = 0: d = inf, d * Kinv has 0 * inf = NaN -> every coordinate NaN; kept (no depth test)
        (2, nan3, n, 0),                        # iD = -0: d = -inf, the same
        (3, (0.5, 2.0625, 2.5), n, 1),          # iD = -2: d = -0.5, Xcam = (-0.5, 0.0625, -0.5)
        (4, big, n, 0),                         # denormal iD
        (5, KAT_T, n, 1),                       # iD = inf: d = 0, Xworld = t
        (7, (2.0, 2.125, 4.0), nan3, 0),        # normal y NaN: kept, R n = NaN in every component (0 * NaN)
        (8, (0.5, 2.375, 4.0), n, 0),
        (9, (1.0, 2.75, 5.0), n, 1),
        (10, (3.0, 3.5, 7.0), n, 0),
        (11, (1.5, 2.1875, 3.5), n, 1),
    ]
    assert got["pixel"].tolist() == [e[0] for e in expect]      # pixel 0 (iD NaN) and 6 (normal x NaN) are skipped
    for g, (p, X, nw, novel) in zip(got, expect):
        np.testing.assert_array_equal([g["x"], g["y"], g["z"]], np.float32(X), err_msg=str(p))
        np.testing.assert_array_equal([g["nx"], g["ny"], g["nz"]], np.float32(nw), err_msg=str(p))
        assert (g["r"], g["g"], g["b"]) == (10 * p, 10 * p + 1, 10 * p + 2) and g["flags"] == novel
    nov = cloud_numpy(block, rows, cols, KAT_K, np.eye(3), KAT_T, "novel")
    assert nov["pixel"].tolist() == [1, 3, 5, 9, 11] and (nov["flags"] == 1).all()
    ok, _ = records_equal(nov, got[got["flags"] == 1])
    assert ok


def test_cloud_numpy_pose_and_order():
    """a rotated pose: every dot product in the fixed order, raster order of the records"""
    rng = np.random.default_rng(5)
    rows, cols = 5, 7
    N = rows * cols
    iD = rng.uniform(0.2, 1.0, N).astype(np.float32); iD[rng.random(N) < 0.3] = np.nan
    nrm = rng.normal(size=(3, N)).astype(np.float32)
    block = make_block(rng.integers(0, 2, N), rng.integers(0, 256, (N, 3)), iD, nrm)
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    t = np.array([0.1, -0.2, 0.3])
    K = (5.5, 6.25, 3.1, 2.2)
    got = cloud_numpy(block, rows, cols, K, R, t, "all")
    Ki = kinv_numpy(K)
    p = int(got["pixel"][3])
    d = np.float64(np.float32(1) / iD[p])
    Xc = [((d * Ki[i, 0]) * (p % cols) + (d * Ki[i, 1]) * (p // cols)) + (d * Ki[i, 2]) * 1.0 for i in range(3)]
    Xw = [((R[i, 0] * Xc[0] + R[i, 1] * Xc[1]) + R[i, 2] * Xc[2]) + t[i] for i in range(3)]
    assert [got["x"][3], got["y"][3], got["z"][3]] == [np.float32(v) for v in Xw]
    assert (np.diff(got["pixel"].astype(np.int64)) > 0).all()
    assert len(got) == int((~np.isnan(iD)).sum())


def test_kinv_formation():
    """the library's Kinv is the restatement's, bit for bit; with K = (2, 4, 1, 0.5) it is exact; Kinv(0, 0) = fy / (fx fy), not 1 / fx"""
    np.testing.assert_array_equal(CL.kinv(KAT_K), [[0.5, 0, -0.5], [0, 0.25, -0.125], [0, 0, 1]])
    for K in [(525.0, 525.0, 319.5, 239.5), (131.25, 131.25, 79.875, 59.875), (517.3, 516.5, 318.6, 255.3), (481.2, -480.0, 319.5, 239.5)]:
        a, b = CL.kinv(K), kinv_numpy(K)
        assert a.tobytes() == b.tobytes(), (K, a, b)
        np.testing.assert_allclose(a @ np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float64), np.eye(3), atol=1e-5)
    fy = np.float64(np.float32(516.5)); fx = np.float64(np.float32(517.3))
    assert kinv_numpy((517.3, 516.5, 0, 0))[0, 0] == fy * (1.0 / (fx * fy))


def test_ply_layout():
    pts = np.zeros(3, CL.POINT_DTYPE)
    pts["x"] = [1.0, -2.5, 0.0]; pts["y"] = [0.5, 3.0, -0.0]; pts["z"] = [2.0, 4.0, 1e-3]
    pts["nx"] = [0.0, 1.0, 0.6]; pts["ny"] = [0.0, 0.0, 0.0]; pts["nz"] = [-1.0, 0.0, -0.8]
    pts["pixel"] = [7, 9, 12]; pts["r"] = [255, 1, 2]; pts["g"] = [0, 3, 4]; pts["b"] = [128, 5, 6]; pts["flags"] = [1, 0, 1]
    head = (b"ply\nformat binary_little_endian 1.0\ncomment rgbid keyframe point cloud\nelement vertex 3\n"
            b"property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    body = b"".join(struct.pack("<6f3B", *[float(pts[f][i]) for f in ("x", "y", "z", "nx", "ny", "nz")], *[int(pts[c][i]) for c in "rgb"])
                    for i in range(3))
    assert len(body) == 3 * 27
    got = CL.ply_bytes(pts)
    assert got == head + body
    assert CL.ply_bytes(pts.view(np.uint8).reshape(3, 32)) == got        # the [M, 32] byte records give the same file
    assert CL.ply_bytes(np.zeros(0, CL.POINT_DTYPE)) == head.replace(b"vertex 3", b"vertex 0")


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_cloud.c"
    src.write_text('#include "rgbid_cloud.h"\n'
                   "typedef char point_is_32_bytes[sizeof(rgbid_cloud_point) == 32 ? 1 : -1];\n"
                   "int use(rgbid_cloud* c) { unsigned long long off[2]; return rgbid_cloud_plan(c, 0, 0, 0, RGBID_CLOUD_NOVEL_ONLY, off); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_cloud_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_cloud.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_cloud_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(CL.EXPORTS), set(declared) ^ set(CL.EXPORTS)
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing
