"""CPU checks of the multi-level feature extractor (include/rgbid_loopfeat.h "levels", rgbid.loopfeat): the library's host side (resize
tables, level geometry, budget per level, refusals) against the numpy restatement tests/loopfeat_levels_mirror.py and against values worked
out by hand; the restatement at one level against the single-level one; and the need itself: a revisit at 1.6 x the distance that one level
loses and eight levels close."""
import ctypes

import numpy as np
import pytest

from rgbid import _lib
from rgbid import loopfeat as LF
from tests import loopfeat_levels_mirror as ML
from tests import loopfeat_mirror as M

SIZES = [(480, 640), (240, 320), (120, 160), (97, 131)]
SCALES = [1.2, 1.5, 2.0]


def test_resize_table_by_hand():
    """4 -> 2 pixels: fx = (d + 0.5) 2 - 0.5 = 0.5, 2.5: x0 = 0, 2 and w1 = 1024.  3 -> 2: fx = 0.25, 1.75: w1 = 512, 1536.  5 -> 4: the first
    centre is at 0.125 (w1 = 256), the last at 3.875 (x0 = 3, w1 = 1792).  Enlarging 2 -> 4 clamps both ends: fx = -0.25 gives (0, 0), fx =
    1.25 gives x0 = 1 = src - 1 and so (1, 0).  A pixel: rows 0, 1 = (0, 100), (200, 44) at weights 1024 give (0 + 100 + 200 + 44) / 4 = 86."""
    for (src, dst), want in {(4, 2): ([0, 2], [1024, 1024]), (3, 2): ([0, 1], [512, 1536]), (5, 4): ([0, 1, 2, 3], [256, 768, 1280, 1792]),
                             (2, 4): ([0, 0, 0, 1], [0, 512, 1536, 0])}.items():
        for x0, w1 in (ML.resize_table(src, dst), LF.resize_table(src, dst)):
            assert x0.tolist() == want[0] and w1.tolist() == want[1], (src, dst, x0, w1)
    assert ML.resize(np.array([[0, 100], [200, 44]], np.uint8), 1, 1).tolist() == [[86]]
    img = np.full((40, 50), 255, np.uint8)
    assert (ML.resize(img, 33, 41) == 255).all() and (ML.resize(np.zeros((40, 50), np.uint8), 33, 41) == 0).all()


@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("scale", SCALES)
def test_library_tables_geometry_and_layout_equal_mirror(rows, cols, scale):
    """resize tables of every level and axis, level sizes, s_l, cells and per-cell budgets: the C library, the Python twin and the mirror agree"""
    want = ML.budget(rows, cols, 1000, 8, scale)
    assert want is not None
    assert LF.plan_levels(rows, cols, 1000, 8, scale) == want
    assert LF.layout_levels(rows, cols, 1000, 8, scale) == want
    geo = ML.geometry(rows, cols, 8, scale)
    assert [(g[0], g[1]) for g in geo] == [(w[0], w[1]) for w in want] and geo[0][:2] == (rows, cols) and geo[0][2] == 1.0
    assert all(w[0] >= 33 and w[1] >= 33 for w in want)
    if len(want) < 8:      # the next level would be too small
        s = np.float32(np.float32(scale) ** len(want))
        assert min(int((rows + 0.5) / s), int((cols + 0.5) / s)) < 33
    for a, b in zip(want[:-1], want[1:]):
        for axis in (0, 1):
            x0, w1 = LF.resize_table(a[axis], b[axis])
            mx0, mw1 = ML.resize_table(a[axis], b[axis])
            assert np.array_equal(x0, mx0) and np.array_equal(w1, mw1)
            assert x0.min() >= 0 and x0.max() <= a[axis] - 1 and w1.min() >= 0 and w1.max() <= 2048
    for levels in (1, 3):
        assert LF.plan_levels(rows, cols, 1000, levels, scale) == ML.budget(rows, cols, 1000, levels, scale) == LF.layout_levels(rows, cols, 1000, levels, scale)


def test_budget_by_hand():
    """320 x 240, 1000 keypoints, 8 levels at 1.2: r = 1 / 1.44, shares 1000 (1 - r) r^l / (1 - r^8) = 323, 224, 155, 108, 75, 52, 36, 25 over
    80, 63, 42, 30, 20, 12, 12, 9 cells (level 1 is 267 x 200: 9 x 7): 4, 3, 3, 3, 3, 4, 3, 2 per cell (integer division, at least 1), 887 slots.  640 x 480: level 5 is
    (int) (640.5 / 2.48832) x (int) (480.5 / 2.48832) = 257 x 193, 9 x 7 cells; one per cell on every level, 300 + 221 + 154 + 108 + 80 + 63 +
    35 + 30 = 991 slots.  One level: per_cell = max_keypoints / cells exactly, as rgbid.loopfeat.layout."""
    p = LF.plan_levels(240, 320, 1000, 8, 1.2)
    assert [q[2] * q[3] for q in p] == [80, 63, 42, 30, 20, 12, 12, 9]
    assert [q[4] for q in p] == [4, 3, 3, 3, 3, 4, 3, 2] and sum(q[2] * q[3] * q[4] for q in p) == 887
    p = LF.plan_levels(480, 640, 1000, 8, 1.2)
    assert (p[5][0], p[5][1]) == (193, 257) and [q[4] for q in p] == [1] * 8 and sum(q[2] * q[3] * q[4] for q in p) == 991
    assert (p[7][0], p[7][1]) == (134, 178)     # (int) (480.5 / 3.58318) = 134
    for rows, cols, mk in ((480, 640, 1000), (120, 160, 1000), (64, 64, 1536), (97, 131, 400), (240, 320, 600), (33, 40, 4)):
        cx, cy, k = LF.layout(rows, cols, mk)
        assert LF.plan_levels(rows, cols, mk, 1, 1.2) == [(rows, cols, cx, cy, k, 1.0)] == LF.layout_levels(rows, cols, mk)


def test_refusals_without_device():
    """levels 0 and 9, scale 1.0 (and NaN, 2.5), a budget that does not fit: RGBID_E_INVALID in C, ValueError in Python; NULL handles"""
    from rgbid._lib import RgbidError
    bad = [(480, 640, 1000, 0, 1.2), (480, 640, 1000, 9, 1.2), (480, 640, 1000, 8, 1.0), (480, 640, 1000, 2, float("nan")),
           (480, 640, 1000, 2, 2.5), (480, 640, 900, 8, 1.2), (480, 640, 299, 1, 1.2), (32, 64, 100, 1, 1.2), (64, 64, 1537, 1, 1.2)]
    for args in bad:
        with pytest.raises(ValueError):
            LF.layout_levels(*args)
        with pytest.raises(RgbidError):
            LF.plan_levels(*args)
    assert ML.budget(480, 640, 900, 8, 1.2) is None and ML.budget(480, 640, 991, 8, 1.2) is not None
    assert len(LF.plan_levels(480, 640, 991, 8, 1.2)) == 8
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.rgbid_loopfeat_create_levels.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_float]
    L.rgbid_loopfeat_plan_levels.argtypes = [ci, ci, ci, ci, ctypes.c_float, vp, vp, vp]
    h = ctypes.c_void_p()
    assert L.rgbid_loopfeat_create_levels(ctypes.byref(h), None, 480, 640, 1000, 8, ctypes.c_float(1.2)) == -1 and not h.value
    assert L.rgbid_loopfeat_plan_levels(480, 640, 1000, 9, ctypes.c_float(1.2), None, None, None) == -1
    assert L.rgbid_loopfeat_plan_levels(480, 640, 1000, 8, ctypes.c_float(1.0), None, None, None) == -1
    assert L.rgbid_loopfeat_plan_levels(480, 640, 1000, 8, ctypes.c_float(1.2), None, None, None) == 0
    assert L.rgbid_loopfeat_resize_table(0, 4, None, None) == -1
    assert L.rgbid_loopfeat_level_layout(None, 0, None, None, None, None, None, None) == -1
    assert L.rgbid_loopfeat_extract_levels(None, None, None, 1, None, None, None, None) == -1
    assert L.rgbid_loopfeat_pyramid(None, None, 1, 0, None) == -1
    assert L.rgbid_loopfeat_timing_pyramid(None, None) == -1


def test_mirror_at_one_level_is_the_single_level_mirror():
    """levels = 1 gives exactly loopfeat_mirror.extract's records, with depth holes, on two sizes; the aux records repeat x, y at level 0"""
    from tests.test_gpu_loopfeat import K_of, textured
    for rows, cols, mk in ((120, 160, 1000), (97, 131, 400)):
        r = np.random.default_rng(rows)
        g, w = textured(r, rows, cols)
        want, n = M.extract(g, w, K_of(rows, cols), mk)
        rec, aux, k = ML.extract(g, w, K_of(rows, cols), mk, 1, 1.2)
        assert k == n and n > 0 and rec.tobytes() == want.tobytes()
        assert np.array_equal(aux["lx"][:k], rec["x"][:k]) and np.array_equal(aux["px"][:k], rec["x"][:k].astype(np.float32))
        assert not aux["level"].any() and not aux[k:].tobytes().strip(b"\0")


def test_levels_close_a_loop_that_one_level_loses():
    """The scale-change pair: the default synthetic scene at 320 x 240, noise-free, seen from t = (0.05, -0.03, 0) and from 0.75 m closer (median
    depth ratio 1.59).  Mirror match + RANSAC (168 iterations, the reference's seed) + the host gate (10 inliers, hull 0.05): one level fails,
    eight levels at 1.2 pass and the RANSAC pose is within the dense verifier's gate (0.1 m, 0.1 rad: what loop_constraints lets a guess be
    corrected by) of the truth.  Measured with this mirror: one level 574 / 521 keypoints,
    47 matches, 0 inliers; eight levels 697 / 694 keypoints, 161 matches, 27 inliers, translation error 1.9 mm."""
    greys, ws, _, (R, t) = ML.scale_change_pair(0.75)
    tables = (M.rotated(), M.bounds())
    out = {}
    for levels in (1, 8):
        ka, xa, na = ML.extract(greys[0], ws[0], ML.PAIR_K, 1000, levels, 1.2, tables)
        kb, xb, nb = ML.extract(greys[1], ws[1], ML.PAIR_K, 1000, levels, 1.2, tables)
        g = ML.appearance_gate(ka, na, kb, nb)
        print(f"levels {levels}: keypoints {na}, {nb}; matches {len(g['matches'])}; inliers {g['inliers']}; hull {g['hull_query']:.3f} / "
              f"{g['hull_candidate']:.3f}; gate {'passes' if g['ok'] else 'fails'}")
        out[levels] = (g, xa, xb)
    assert not out[1][0]["ok"]
    g, xa, xb = out[8]
    assert g["ok"] and g["inliers"] >= LF.MIN_INLIERS and not g["ransac"]["fragile"]
    Rr, tr = g["ransac"]["R"], g["ransac"]["t"]
    angle = float(np.arccos(np.clip((np.trace(R.T @ Rr) - 1.0) / 2.0, -1.0, 1.0)))
    print(f"RANSAC pose against the truth: {np.linalg.norm(tr - t):.4f} m, {angle:.4f} rad")
    assert np.linalg.norm(tr - t) < 0.1 and angle < 0.1
    # the inlier matches pair the closer view's upper levels with the farther view's lower ones: the depth ratio 1.59 is 1.2^2.5, and a
    # descriptor bears about one level of scale error (one level alone already fails at 1.29 = 1.2^1.4), so the median step is 1 .. 4 levels
    sel = g["matches"][g["ransac"]["mask"].astype(bool)]
    lq, lc = xb["level"][sel["query"]], xa["level"][sel["train"]]
    print("inlier levels (closer, farther):", sorted(zip(lq.tolist(), lc.tolist())))
    assert 1 <= float(np.median(lq.astype(int) - lc.astype(int))) <= 4
