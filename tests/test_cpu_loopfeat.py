"""CPU checks of the loop-feature stage (include/rgbid_loopfeat.h, rgbid.loopfeat): the numpy restatement the GPU tests compare the kernels
against (tests/loopfeat_mirror.py) on hand-computed cases and against plain loops; the library's host tables; the MT19937 draws; the host
side of the proposal and of the gates; the header as C99; the library's exports; refusals that need no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import loopfeat as LF
from tests import loopfeat_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_harris_expression_by_hand():
    """a vertical step edge of height 10 with one corner: at a pixel whose 7 x 7 block holds only the vertical edge, Ix = 40 on the two
    columns beside the step and Iy = 0, so sxx = 14 * 1600 = 22400, syy = sxy = 0 and the response is -(0.04 * 22400 * 22400) * scale4 < 0"""
    g = np.zeros((40, 40), np.uint8)
    g[:, 20:] = 10
    r = M.harris(g)
    f = np.float32
    scale = f(1.0) / (f(28) * f(255.0))
    scale4 = ((scale * scale) * scale) * scale
    want = (f(0.0) - f(0.0)) - ((f(0.04) * f(22400.0)) * f(22400.0)) * scale4
    assert r[20, 20] == want and r[20, 20] < 0
    assert r[20, 10] == 0 and r[2, 20] == 0                      # flat region; within 4 of the border
    # products beyond int32: sxx = syy = 49 * 1020^2 on a checkerboard of 0 / 255 would overflow an int product; here the int64 form is exact
    sxx = 49 * 1020 * 1020
    assert np.float32(sxx * sxx) == np.float32(float(sxx) ** 2) and sxx * sxx > 2 ** 31


def harris_loops(g):
    rows, cols = g.shape
    out = np.zeros((rows, cols), np.float32)
    f = np.float32
    scale = f(1.0) / (f(28) * f(255.0))
    scale4 = ((scale * scale) * scale) * scale
    v = lambda y, x: int(g[y, x])
    for y in range(4, rows - 4):
        for x in range(4, cols - 4):
            sxx = syy = sxy = 0
            for j in range(-3, 4):
                for i in range(-3, 4):
                    yy, xx = y + j, x + i
                    Ix = 2 * (v(yy, xx + 1) - v(yy, xx - 1)) + (v(yy - 1, xx + 1) - v(yy - 1, xx - 1)) + (v(yy + 1, xx + 1) - v(yy + 1, xx - 1))
                    Iy = 2 * (v(yy + 1, xx) - v(yy - 1, xx)) + (v(yy + 1, xx - 1) - v(yy - 1, xx - 1)) + (v(yy + 1, xx + 1) - v(yy - 1, xx + 1))
                    sxx += Ix * Ix; syy += Iy * Iy; sxy += Ix * Iy
            tr = f(sxx + syy)
            out[y, x] = (f(sxx * syy) - f(sxy * sxy)) - ((f(0.04) * tr) * tr) * scale4
    return out


def test_detector_against_plain_loops():
    """response, local maxima with the raster tie-break, per-cell selection and order: the vectorised mirror against loops on a 40 x 48 image
    with plateaus (equal responses side by side)"""
    r = np.random.default_rng(3)
    rows, cols = 40, 48
    g = np.repeat(np.repeat(r.integers(0, 256, (rows // 4, cols // 4)), 4, 0), 4, 1).astype(np.uint8)   # 4 x 4 blocks: many ties
    w = np.ones((rows, cols), np.float32)
    w[18, :24] = np.nan
    resp = M.harris(g)
    assert np.array_equal(resp, harris_loops(g))
    ok = M.local_maxima(resp, w)
    B = LF.BORDER
    want = []
    for y in range(B, rows - B):
        for x in range(B, cols - B):
            c = resp[y, x]
            if not c > 0 or not (np.isfinite(w[y, x]) and w[y, x] > 0):
                continue
            best = all(c > resp[y + dy, x + dx] or (c == resp[y + dy, x + dx] and (dy, dx) > (0, 0))
                       for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
            if best:
                want.append((x, y))
    assert sorted(want) == sorted((int(x), int(y)) for y, x in zip(*np.nonzero(ok)))
    for max_kp in (4, 8, 200):
        cx, cy, k = LF.layout(rows, cols, max_kp)
        sel = []
        for j in range(cy):
            for i in range(cx):
                cell = [(x, y) for x, y in want if x // 32 == i and y // 32 == j]
                cell.sort(key=lambda p: (-float(resp[p[1], p[0]]), p[1] * cols + p[0]))
                sel += cell[:k]
        assert M.select(resp, ok, max_kp) == sel
    assert len(want) >= 2


def test_direction_bins_by_hand():
    """a bright half plane to the right of the keypoint gives m01 = 0, m10 > 0: bin 0; below (y grows downwards): bin 8; left: 16; above: 24;
    a diagonal half plane x + y > 0: bin 4; m10 = m01 = 0 on a constant patch: bin 0.  The boundary vectors never give an exact zero."""
    bnd = M.bounds()
    yy, xx = np.mgrid[0:33, 0:33] - 16
    for cond, want in ((xx > 0, 0), (yy > 0, 8), (xx < 0, 16), (yy < 0, 24), (xx + yy > 0, 4), (xx > 40, 0)):
        g = np.where(cond, 200, 0).astype(np.uint8)
        b, m10, m01 = M.direction(g, 16, 16, bnd)
        assert b == want, (want, b, m10, m01)
    # one step past a boundary: tan(pi / 32) = 0.0985: (m10, m01) = (1000, 98) is bin 0, (1000, 99) is bin 1
    def bin_of(m10, m01):
        upper = m01 > 0 or (m01 == 0 and m10 >= 0)
        mx, my = (m10, m01) if upper else (-m10, -m01)
        return (int(np.sum(bnd[:, 0] * my - bnd[:, 1] * mx > 0.0)) + (0 if upper else 16)) & 31
    assert (bin_of(1000, 98), bin_of(1000, 99), bin_of(1000, -98), bin_of(1000, -99), bin_of(-1000, 0), bin_of(0, -5)) == (0, 1, 0, 31, 16, 24)
    for m10 in range(-60, 61):
        for m01 in range(-60, 61):
            want = int(np.floor(np.arctan2(m01, m10) / (np.pi / 16) + 0.5)) % 32 if (m10 or m01) else 0
            assert bin_of(m10, m01) == want, (m10, m01)


def test_tables_equal_the_librarys_and_descriptor_byte():
    """the seeded recipe gives the library's pattern, rotated tables and bin boundaries bit for bit; every rotated position stays within 13
    (+ the 5 x 5 box: inside the 33 x 33 patch), no rotated coordinate is closer than 1e-5 to a rounding boundary; one descriptor byte by hand"""
    pat, rot, bnd = LF.tables()
    assert np.array_equal(pat, M.pattern()) and np.array_equal(rot, M.rotated()) and np.array_equal(bnd, M.bounds())
    assert np.array_equal(rot[0], pat) and np.abs(rot).max() <= 13 and M.rotation_margin() > 1e-5
    assert np.array_equal(rot[8][:, 0], -pat[:, 1]) and np.array_equal(rot[8][:, 1], pat[:, 0])     # a quarter turn, exactly
    assert len({tuple(p) for p in pat.tolist()}) == 256
    g = np.zeros((33, 33), np.uint8)
    g[:, 17:] = 100                                # brighter to the right: bit t is set when x1 + 2 < 17 - 16 + ... i.e. box(p1) < box(p2)
    box = M.box_sums(g)
    d = M.descriptor(box, 16, 16, rot[0])
    cover = lambda x: int(np.clip(x + 2, 0, 5)) if x <= 2 else 5        # columns of the box right of the edge: x - 2 .. x + 2 versus > 0
    cols_right = lambda x: sum(1 for c in range(x - 2, x + 3) if c > 0)
    byte0 = sum(1 << t for t in range(8) if cols_right(int(pat[t, 0])) < cols_right(int(pat[t, 2])))
    assert d[0] == byte0 and d.shape == (32,)


def test_two_nearest_order_on_ties():
    """equal distances: the lower candidate index comes first, as BFMatcher's knnMatch orders them; the ratio test in float32; a candidate
    with one keypoint gives nothing"""
    kq = np.zeros(3, LF.KP_DTYPE); kc = np.zeros(4, LF.KP_DTYPE)
    kc["desc"][0, 0] = 0b00000111      # distance 3 from a zero query
    kc["desc"][1, 0] = 0b00000001      # 1
    kc["desc"][2, 1] = 0b00010000      # 1: a tie with candidate 1
    kc["desc"][3, :] = 255             # 256
    kq["desc"][1, :] = 255             # nearest 3 (d 0), second 0 (d 253)
    kq["desc"][2, 0] = 0b00000110      # distances 1, 3, 3, 254: nearest 0, second 3
    m = M.match(kq, 3, kc, 4)
    assert m.tolist() == [(1, 3, 0, 253), (2, 0, 1, 3)]          # query 0: d0 = d1 = 1 fails 1 < 0.75 * 1
    m = M.match(kq, 3, kc, 4, ratio=1.5)
    assert m.tolist() == [(0, 1, 1, 1), (1, 3, 0, 253), (2, 0, 1, 3)]
    assert len(M.match(kq, 3, kc, 1, ratio=1.5)) == 0 and len(M.match(kq, 0, kc, 4)) == 0
    assert not np.float32(3) < np.float32(0.75) * np.float32(4) and np.float32(2) < np.float32(0.75) * np.float32(3)


def test_mt19937_draws_and_iterations():
    """numpy's RandomState seeds by init_genrand as boost::mt19937 does: seed 5489 gives the published first outputs; the draws are x / 2^32;
    the iteration count in float32"""
    rs = np.random.RandomState(5489)
    assert LF.mt19937_words(rs, 2).tolist() == [3499211612, 581869302]
    u = LF.uniform_draws(2, seed=5489)
    assert u[0] == 3499211612 / 2.0 ** 32 and u[1] == 581869302 / 2.0 ** 32 and len(u) == 6
    u = LF.uniform_draws(168)
    assert (u >= 0).all() and (u < 1).all() and np.array_equal(u[:9], LF.uniform_draws(3))
    assert LF.num_iters() == 168
    assert int(np.log(1 - 0.99) / np.log(1 - 0.3 ** 3) - 1) + 1 == 168


def test_sampling_replay_by_hand():
    """selectRandomMatches on 5 matches with u = 0.5, 0.6, 0.7: (int) 2.5 = 2 -> entry 2, list 0 1 4 3; (int) 2.4 = 2 -> entry 4, list 0 1 3;
    (int) 2.1 = 2 -> entry 3"""
    assert M.sample3([0.5, 0.6, 0.7], 5) == [2, 4, 3]
    assert M.sample3([0.99, 0.0, 0.0], 3) == [2, 0, 1]
    assert M.sample3([0.0, 0.0, 0.0], 4) == [0, 3, 2]


def test_pose_and_vote_by_hand():
    """a quarter turn about z and a shift: three exact correspondences give it back (SVD and Horn); a reflected triangle still gives a proper
    rotation; one vote: a point 3 sigma off along x is an inlier of the 4.11 threshold, 5 sigma off is not"""
    Rt = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]); tt = np.array([0.5, -0.25, 0.125])
    C = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.5], [0.0, 2.0, 2.0]])
    Q = C @ Rt.T + tt
    for f in (M.pose3_svd, M.pose3_horn):
        R, t = f(Q, C)
        assert np.allclose(R, Rt, atol=1e-14) and np.allclose(t, tt, atol=1e-14)
    Qm = Q * np.array([1.0, 1.0, -1.0])            # mirrored: no rotation maps the triangles onto each other with their normals
    R1, _ = M.pose3_svd(Qm, C); R2, _ = M.pose3_horn(Qm, C)
    assert abs(np.linalg.det(R1) - 1) < 1e-12 and np.allclose(R1, R2, atol=1e-12)
    cov = np.array([[1e-6, 0, 0, 1e-6, 0, 1e-6]])  # sigma 1 mm in both keyframes: total sigma sqrt(2) mm
    I, z = np.eye(3), np.zeros(3)
    X = np.array([[0.1, 0.2, 1.0]])
    s = np.sqrt(2.0) * 1e-3
    e3 = M.errors3d(X, cov, X + [3 * s, 0, 0], cov, I, z)[0]
    e5 = M.errors3d(X, cov, X + [5 * s, 0, 0], cov, I, z)[0]
    assert abs(e3 - 3.0) < 1e-9 and abs(e5 - 5.0) < 1e-9 and e3 < LF.MAHALANOBIS_TH < e5


def test_mirror_ransac_is_not_fragile_on_the_committed_seeds():
    """the GPU test may leave out a pair only when the mirror sees an error within 1e-6 of the threshold in a near-best hypothesis, and at most
    5 % of the pairs: on the committed seeds the mirror alone flags none (measured: 0 of 64), and it recovers the true pose"""
    from tests.test_gpu_loopfeat import GUARD, MAX_LEFT_OUT, RANSAC_SEEDS, synthetic_pairs
    u = LF.uniform_draws(LF.num_iters())
    data = synthetic_pairs()
    res = [M.ransac(kq, kc, m, u, guard=GUARD) for kq, kc, m, _ in data]
    fragile = sum(1 for r in res if r["fragile"])
    print(f"{fragile} of {len(res)} pairs fragile; inliers {min(r['inliers'] for r in res)} .. {max(r['inliers'] for r in res)}")
    assert fragile <= MAX_LEFT_OUT * len(RANSAC_SEEDS) and fragile == 0
    for r, (_, _, _, (R, t)) in zip(res, data):
        assert r["best"] >= 0 and r["inliers"] >= 10
        assert np.abs(r["R"] - R).max() < 0.05 and np.abs(r["t"] - t).max() < 0.05


def test_selection_and_gates():
    """the proposal's host side: normalisation by the previous keyframe, threshold, 2 of largest separation then 2 of best score without
    duplicates; the hull area by the reference's trapezoid formula; the inlier and hull gates"""
    counts = {(5, 4): 100, (5, 0): 70, (5, 1): 61, (5, 2): 90, (4, 3): 100, (4, 0): 60, (4, 1): 59, (3, 2): 0, (3, 0): 50}
    pairs, scores = LF.select_candidates(6, counts, min_separation=3)
    # q = 5: 0.7, 0.61, 0.9 pass; separation picks 0, 1; score picks 2 (and 0 again).  q = 4: 60 / 100 is not > 0.6 in float32; q = 3: no reference
    assert pairs == [(5, 0), (5, 1), (5, 2)] and abs(scores[(5, 2)] - 0.9) < 1e-6
    pairs, _ = LF.select_candidates(6, counts, min_separation=3, score_threshold=0.595)
    assert pairs == [(4, 0), (5, 0), (5, 1), (5, 2)]
    counts.update({(6, 5): 10, (6, 0): 7, (6, 1): 8, (6, 2): 9, (6, 3): 9})
    assert LF.select_candidates(7, counts)[0][-4:] == [(6, 0), (6, 1), (6, 3), (6, 2)]     # separation 0, 1; then score 0.9: the later one first
    assert LF.all_pairs(5, 3) == [(1, 0), (2, 1), (3, 2), (3, 0), (4, 3), (4, 0), (4, 1)]
    assert LF.hull_area([(0, 0), (4, 0), (4, 3), (0, 3), (2, 1), (4, 3)]) == 12.0 and LF.hull_area([(0, 0), (1, 1), (2, 2)]) == 0.0
    kq = np.zeros(12, LF.KP_DTYPE); kc = np.zeros(12, LF.KP_DTYPE)
    pts = [(0, 0), (100, 0), (100, 100), (0, 100)] + [(10 + i, 20 + 2 * i) for i in range(8)]
    kq["x"], kq["y"] = zip(*pts); kc["x"], kc["y"] = zip(*pts)
    m = np.zeros(12, LF.MATCH_DTYPE); m["query"] = m["train"] = np.arange(12)
    ok, inl, hq, hc = LF.gate(kq, kc, m, np.ones(12, np.uint8), 200, 200)
    assert ok and inl == 12 and hq == hc == 0.25
    assert not LF.gate(kq, kc, m, np.ones(12, np.uint8), 480, 640)[0]                    # 10 000 / 307 200 < 0.05
    mask = np.ones(12, np.uint8); mask[:3] = 0
    assert not LF.gate(kq, kc, m, mask, 200, 200)[0]                                     # 9 inliers


def test_layout_and_refusals_without_device():
    assert LF.layout(480, 640, 1000) == (20, 15, 3) and LF.layout(120, 160, 1000) == (5, 4, 50) and LF.layout(64, 64, 1536) == (2, 2, 64)
    for bad in ((32, 64, 100), (480, 640, 299), (64, 64, 1537), (9000, 64, 1000)):
        with pytest.raises(ValueError):
            LF.layout(*bad)
    L = _lib_handle()
    h = ctypes.c_void_p()
    L.rgbid_loopfeat_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert L.rgbid_loopfeat_create(ctypes.byref(h), None, 480, 640, 1000) == -1 and not h.value
    assert L.rgbid_loopfeat_create(None, None, 480, 640, 1000) == -1
    assert L.rgbid_loopfeat_destroy(None) == 0
    assert L.rgbid_loopfeat_extract(None, None, None, 1, None, None, None) == -1
    assert L.rgbid_loopfeat_match(None, None, None, 0, None, 0, ctypes.c_float(0.75), None, None) == -1
    assert L.rgbid_loopfeat_timing(None, 0, None) == -1


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_loopfeat.c"
    src.write_text('#include "rgbid_loopfeat.h"\n'
                   "#include <stddef.h>\n"
                   "typedef char kp_is_120_bytes[sizeof(rgbid_loopfeat_kp) == 120 ? 1 : -1];\n"
                   "typedef char desc_at_16[offsetof(rgbid_loopfeat_kp, desc) == 16 && offsetof(rgbid_loopfeat_kp, X) == 48 ? 1 : -1];\n"
                   "typedef char corr_is_16_bytes[sizeof(rgbid_loopfeat_corr) == 16 ? 1 : -1];\n"
                   "int use(rgbid_loopfeat* f, const rgbid_loopfeat_kp* k, const int32_t* c, const int32_t* p, int32_t* n) {\n"
                   "  return rgbid_loopfeat_match(f, k, c, 2, p, 1, 0.75f, NULL, n); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_loopfeat_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_loopfeat.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_loopfeat_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(LF.EXPORTS), set(declared) ^ set(LF.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_loop_constraints_guess_argument_is_checked():
    from rgbid import posegraph as PG
    with pytest.raises(ValueError):
        PG.loop_constraints(None, [dict(frame=0), dict(frame=5)], None, None, None, pairs=[(1, 0)], guess=[])
    with pytest.raises(ValueError):
        PG.optimise_run(None, np.zeros((1, 3, 3)), np.zeros((1, 3)), [], [], [], [], None, loops="orb")
