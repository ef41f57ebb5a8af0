"""CPU checks of the colour alignment contract (include/rgbid_colouralign.h): the mirror against hand-written
values, against a finite difference of its own residual, against the scalar restatement of one pair and on the scene the operator was
prototyped on; the Python layer's checkers, the header as C99 and the library's exports.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from rgbid import _lib
from rgbid import colouralign as CA
from rgbid import recolour as RC
from tests import align_mirror as AM
from tests import colouralign_mirror as CM
from tests.render_mirror import pose_cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
UNIT = (1.0, 1.0, 0.0, 0.0)              # with Z = 1 and the identity pose u = x and v = y exactly: a vertex is given in pixels
PRM = dict(CM.PARAMS, z_min=0.5, z_max=4.0)
IDENTITY = pose_cw(np.eye(3), np.zeros(3))


def at_pixels(x, y):
    return np.array([[x, y, 1.0]], F)


# ---- step 4 by hand -----------------------------------------------------------------------------------------------------------------------
def test_the_grey_sample_of_a_two_by_two_image():
    """L = 77 R + 150 G + 29 B: 4 640, 31 850, 38 250, 65 280; at ax = 64, ay = 192 the weights are 12 288, 4 096, 36 864, 12 288"""
    img = np.array([[[10, 20, 30], [200, 100, 50]], [[0, 255, 0], [255, 255, 255]]], np.uint8)
    assert list(CM.grey_plane(img)) == [4640, 31850, 38250, 65280]
    pv = CM.pair_values(at_pixels(64 / 256, 192 / 256), None, IDENTITY, UNIT, 2, 2, img, None, None, PRM)
    assert list(pv["taken"]) == [0] and int(pv["w"][0]) == 1024
    s = 12288 * 4640 + 4096 * 31850 + 36864 * 38250 + 12288 * 65280
    Gx = 64 * (31850 - 4640) + 192 * (65280 - 38250)
    Gy = 192 * (38250 - 4640) + 64 * (65280 - 31850)
    assert (s, Gx, Gy) == (2399682560, 6931200, 8592640)
    assert (int(pv["s"][0]), int(pv["Gx"][0]), int(pv["Gy"][0])) == (s, Gx, Gy)
    # g, dx, dy are exact: the divisors are powers of two
    assert pv["s"].astype(D)[0] / 16777216.0 == 143.03222656250 and Gx / 65536.0 == 105.76171875 and Gy / 65536.0 == 131.11328125
    # the last column, the last row, a 1 x 1 image: the differences vanish by themselves
    pv = CM.pair_values(at_pixels(1.0, 0.25), None, IDENTITY, UNIT, 2, 2, img, None, None, PRM)
    assert int(pv["Gx"][0]) == 0 and int(pv["Gy"][0]) == 256 * (65280 - 31850) and int(pv["s"][0]) == 65536 * 31850 + 64 * 256 * (65280 - 31850)
    pv = CM.pair_values(at_pixels(0.5, 1.0), None, IDENTITY, UNIT, 2, 2, img, None, None, PRM)
    assert int(pv["Gy"][0]) == 0 and int(pv["Gx"][0]) == 256 * (65280 - 38250)
    pv = CM.pair_values(at_pixels(0.0, 0.0), None, IDENTITY, UNIT, 1, 1, img[:1, :1], None, None, PRM)
    assert (int(pv["s"][0]), int(pv["Gx"][0]), int(pv["Gy"][0])) == (65536 * 4640, 0, 0)
    # half a lattice step beyond the last texel is outside
    assert not len(CM.pair_values(at_pixels(1.0 + 1 / 256, 0.0), None, IDENTITY, UNIT, 2, 2, img, None, None, PRM)["taken"])


def test_the_target_of_weights_1024_and_512():
    """view 0 faces the vertex (cos = 1, w = 1 024) and shows grey 100, view 1 sees it under 60 degrees (cos = 0.5, w = 512) and shows
    grey 40: S = (1 024 * 100 + 512 * 40) * 256 * 65 536, W = 1 536, C = 122 880 / 1 536 = 80 exactly"""
    pos, nrm = np.array([[0.0, 0.0, 1.0]], F), np.array([[0.0, 0.0, -1.0]], F)
    R1, t1 = CM.look_at((np.sqrt(3.0), 0.0, 0.0), (0.0, 0.0, 1.0))
    K = (50.0, 50.0, 7.5, 7.5)
    ms = [IDENTITY, pose_cw(R1, t1)]
    cols = [np.full((16, 16, 3), 100, np.uint8), np.full((16, 16, 3), 40, np.uint8)]
    S, W, used = CM.targets(pos, nrm, ms, K, 16, 16, cols, None, None, PRM)
    assert int(W[0]) == 1536 and int(used[0]) == 2 and int(S[0]) == (1024 * 100 + 512 * 40) * 256 * 65536
    has, C = CM.target_values(S, W, used, 2)
    assert has[0] and C[0] == 80.0
    assert not CM.target_values(S, W, used, 3)[0][0]
    # one view alone is no target under min_views = 2
    S, W, used = CM.targets(pos, nrm, ms[:1], K, 16, 16, cols[:1], None, None, PRM)
    assert int(W[0]) == 1024 and not CM.target_values(S, W, used, 2)[0][0]


# ---- step 6: J against a finite difference of the mirror's own f ---------------------------------------------------------------------------
def test_the_jacobian_against_a_central_difference():
    """f = g - C with C held, under the twist that align_mirror.update applies.  The difference quotient over +-h is compared with J for
    the pairs whose footprint is the same texel at 0, +-h and +-2h: there g is the bilinear interpolant of four fixed values, sampled at
    positions snapped to 1/256 pixel.  Its error has two parts.  Snapping: each sample is taken up to 1/512 pixel off in x and in y, so
    each f is off by at most (|dx| + |dy|) / 512 grey levels and the quotient by (|dx| + |dy|) / (512 h) (the float32 projection's
    rounding, 2^-24 of ~100 pixels, is 300 times smaller and is covered by the factor 1.5).  Truncation: the central difference's
    error is h^2 f''' / 6 + O(h^4); the quotient over +-2h has four times that, so |q(2h) - q(h)| = 3 |truncation of q(h)| up to the
    snapping of q(2h), which is half of q(h)'s.  The bound used is 1.5 (|dx| + |dy|) / (512 h) + |q(2h) - q(h)|, which holds both."""
    sc = CM.scene(V=2, size=0.0, nx=140, ny=110)
    pos, K, rows, cols = sc["vertices"], sc["K"], sc["rows"], sc["cols"]
    pose = np.concatenate([sc["R"][1].reshape(9), sc["t"][1]])
    img = sc["colours"][1]
    h = 0.12 * 1.6 / K[0]                                          # about 0.12 pixel per step at the scene's depth

    def sample(delta):
        m = pose_cw(*np.split(AM.update(pose, list(delta)), [9]))
        pv = CM.pair_values(pos, None, m, K, rows, cols, img, None, None, CM.PARAMS)
        g = np.full(len(pos), np.nan)
        g[pv["taken"]] = pv["s"].astype(D) / 16777216.0
        tex = np.full((len(pos), 2), -1)
        tex[pv["taken"]] = np.stack([pv["xs"] >> 8, pv["ys"] >> 8], 1)
        return g, tex, pv, m

    _, tex0, pv0, m0 = sample(np.zeros(6))
    J = CM.jacobian(pv0, pos, m0, K)
    dx, dy = np.abs(pv0["Gx"]) / 65536.0, np.abs(pv0["Gy"]) / 65536.0
    checked = 0
    for k in range(6):
        e = np.zeros(6); e[k] = 1.0
        (gp, tp, _, _), (gm, tm, _, _), (gp2, tp2, _, _), (gm2, tm2, _, _) = sample(h * e), sample(-h * e), sample(2 * h * e), sample(-2 * h * e)
        same = (tex0 >= 0).all(1) & (tp == tex0).all(1) & (tm == tex0).all(1) & (tp2 == tex0).all(1) & (tm2 == tex0).all(1)
        idx = np.flatnonzero(same)
        assert len(idx) > 500, (k, len(idx))
        q1, q2 = (gp - gm)[idx] / (2 * h), (gp2 - gm2)[idx] / (4 * h)
        where = np.searchsorted(pv0["taken"], idx)
        assert (pv0["taken"][where] == idx).all()
        tol = 1.5 * (dx + dy)[where] / (512 * h) + np.abs(q2 - q1)
        err = np.abs(J[k][where] - q1)
        assert (err <= tol).all(), (k, float((err / tol).max()))
        # the bound bites: where the derivative is large, a J of twice the size and one of the wrong sign fail it
        big = np.abs(q1) > np.percentile(np.abs(q1), 75)
        assert (np.abs(2 * J[k][where] - q1) > tol)[big].mean() > 0.9
        assert (np.abs(-J[k][where] - q1) > tol)[big].mean() > 0.9
        checked += len(idx)
    assert checked > 3000


# ---- the mirror against the scalar restatement --------------------------------------------------------------------------------------------
def random_case(seed, n=60, V=3, rows=12, cols=16):
    r = np.random.default_rng(seed)
    K = (14.0, 13.0, 7.3, 5.6)
    pos = np.stack([r.uniform(-0.7, 0.7, n), r.uniform(-0.5, 0.5, n), r.uniform(1.0, 1.2, n)], 1).astype(F)
    nrm = r.normal(size=(n, 3)).astype(F)
    nrm[:, 2] = -np.abs(nrm[:, 2]) - 0.5
    nrm[::7] = 0
    pos[5] = np.nan
    Rs, ts = [], []
    for v in range(V):
        Rv, tv = CM.perturb(np.eye(3), np.zeros(3), 0.1, seed * 10 + v)
        Rs.append(Rv); ts.append(tv)
    colours = [r.integers(0, 256, (rows, cols, 3)).astype(np.uint8) for _ in range(V)]
    surface = [np.where(r.random((rows, cols)) < 0.03, np.nan, 1.1 + r.uniform(-0.2, 0.2, (rows, cols))).astype(F) for _ in range(V)]
    measured = [np.where(r.random((rows, cols)) < 0.03, 0.0, 1.0 / (1.1 + r.uniform(-0.2, 0.2, (rows, cols)))).astype(F) for _ in range(V)]
    prm = dict(CM.PARAMS, z_min=0.5, z_max=4.0, surface_tolerance=0.25, measured_tolerance=0.25, two_sided=bool(seed & 1))
    return dict(pos=pos, nrm=nrm, R=np.stack(Rs), t=np.stack(ts), K=K, rows=rows, cols=cols, colours=colours, surface=surface, measured=measured, prm=prm)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("drop", [(), ("nrm",), ("surface", "measured"), ("nrm", "surface", "measured")])
def test_the_mirror_against_the_scalar_restatement(seed, drop):
    c = random_case(seed)
    for k in drop:
        c[k] = None
    n, V = len(c["pos"]), len(c["R"])
    ms = [pose_cw(c["R"][v], c["t"][v]) for v in range(V)]
    plane = lambda name, v: None if c[name] is None else c[name][v]
    loops = [[CM.pair_loop(c["pos"][i], None if c["nrm"] is None else c["nrm"][i], ms[v], c["K"], c["rows"], c["cols"], c["colours"][v],
                           plane("surface", v), plane("measured", v), c["prm"]) for i in range(n)] for v in range(V)]
    S, W, used = CM.targets(c["pos"], c["nrm"], ms, c["K"], c["rows"], c["cols"], c["colours"], c["surface"], c["measured"], c["prm"])
    for i in range(n):
        got = [l[i] for l in loops if l[i] is not None]
        assert int(used[i]) == len(got) and int(W[i]) == sum(g["w"] for g in got) and int(S[i]) == sum(g["w"] * g["s"] for g in got)
    assert 0 < (used >= 2).sum() < n
    has, C = CM.target_values(S, W, used, 2)
    for huber in (16.0, 0.5):
        for v in range(V):
            u, t = CM.terms(c["pos"], c["nrm"], ms[v], c["K"], c["rows"], c["cols"], c["colours"][v], plane("surface", v), plane("measured", v),
                            c["prm"], has, C, huber)
            for i in range(n):
                want = loops[v][i] is not None and bool(has[i])
                assert bool(u[i]) == want
                if want:
                    one = CM.terms_loop(loops[v][i], c["pos"][i], ms[v], c["K"], C[i], huber)
                    assert np.array(one, D).tobytes() == t[:, i].tobytes(), (v, i)
                else:
                    assert t[:, i].tobytes() == np.zeros(28, D).tobytes()
            # the sums through the explicit loops over the lanes
            n_used, sums, per_group = CM.system(c["pos"], c["nrm"], ms[v], c["K"], c["rows"], c["cols"], c["colours"][v], plane("surface", v),
                                                plane("measured", v), c["prm"], has, C, huber)
            lanes = CM.MR.group_lanes(t)
            assert n_used == int(u.sum()) == int(per_group.sum()) and lanes.shape == (28, 1, 64)
            assert np.array([AM.reduce_loop([AM.tree64_loop(lanes[k, 0])]) for k in range(28)], D).tobytes() == sums.tobytes()


def test_huber_met_exactly_and_one_ulp_either_side():
    """a pair whose |f| is the threshold has wh = 1; one float32 ulp below the threshold it has wh = huber / |f|"""
    pos = np.array([[0.0, 0.0, 1.0]], F)
    K = (50.0, 50.0, 7.5, 7.5)
    img = np.zeros((16, 16, 3), np.uint8); img[:, 8:] = 90
    has, C = np.array([True]), np.array([20.0])
    pv = CM.pair_values(pos, None, IDENTITY, K, 16, 16, img, None, None, PRM)
    f = float(pv["s"][0]) / 16777216.0 - 20.0
    assert f == 25.0                                              # u = 7.5: halfway between grey 0 and 90
    for huber, unit in ((25.0, True), (np.nextafter(F(25), F(30)), True), (np.nextafter(F(25), F(0)), False)):
        _, t = CM.terms(pos, None, IDENTITY, K, 16, 16, img, None, None, PRM, has, C, huber)
        assert (t[27, 0] == f * f) == unit and t[27, 0] == (1.0 if unit else float(D(F(huber)) / 25.0)) * f * f


# ---- the scene the operator was prototyped on ----------------------------------------------------------------------------------------------
def errors(sc, R, t):
    return np.array([CM.pixel_error(sc["vertices"], sc["K"], R[v], t[v], sc["R"][v], sc["t"][v]) for v in range(len(R))])


def test_the_prototype_scene_at_one_scale():
    """a textured plane, 3 850 vertices, six 128 x 96 views, view 0 held, the others perturbed by 0.006: the cost per pair of every moved
    view falls and its mean pixel error to the true pose at least halves (8 rounds x 3 iterations)"""
    sc = CM.scene(size=0.006)
    assert len(sc["vertices"]) == 3850
    before = errors(sc, sc["Rp"], sc["tp"])
    out = CM.run(sc["vertices"], sc["Rp"], sc["tp"], sc["K"], sc["rows"], sc["cols"], sc["colours"], fixed=(0,), rounds=8, iterations=3)
    rec = out["records"]
    after = errors(sc, rec["pose"][:, :9].reshape(-1, 3, 3), rec["pose"][:, 9:])
    cost = CM.cost_per_pair(rec)
    print("pixel error before", before[1:], "after", after[1:], "cost per pair", cost[1:])
    assert rec["status"][0] == CM.FIXED and rec["iterations"][0] == 0 and after[0] == 0 and (rec["iterations"][1:] == 24).all()
    assert (before[1:] > 0.4).all()
    assert (cost[1:, 1] < cost[1:, 0]).all()
    assert (after[1:] <= before[1:] / 2).all(), (before, after)


def test_the_prototype_scene_over_three_scales():
    """the same scene perturbed by 0.02, refined at the scales 4, 2, 1 with 4 rounds x 3 iterations each"""
    sc = CM.scene(size=0.02)
    before = errors(sc, sc["Rp"], sc["tp"])
    R, t, outs = CM.refine(sc["vertices"], sc["Rp"], sc["tp"], sc["K"], sc["rows"], sc["cols"], sc["colours"], scales=(4, 2, 1), fixed=(0,),
                           rounds=4, iterations=3)
    after = errors(sc, R, t)
    print("pixel error before", before[1:], "after", after[1:])
    assert (before[1:] > 1.5).all()
    for o in outs:
        cost = CM.cost_per_pair(o["records"])
        assert (cost[1:, 1] < cost[1:, 0]).all()
    assert (after[1:] <= before[1:] / 2).all(), (before, after)


def test_the_scale_convention():
    """a vertex projects to the same place at the scales 1, 2 and 4: u_f = (u_1 - (f - 1) / 2) / f, so that the centre of the coarse
    pixel p lies over the centre of the fine pixels f p .. f p + f - 1; the box filter takes exactly those"""
    K = (140.8, 139.2, 63.5, 47.25)
    r = np.random.default_rng(1)
    c = np.stack([r.uniform(-0.5, 0.5, 50), r.uniform(-0.4, 0.4, 50), r.uniform(1.0, 2.0, 50)], 1)
    u1 = np.stack([K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], 1)
    for f in (1, 2, 4):
        Kf = CM.scaled_intrinsics(K, f)
        assert Kf == CA.scaled_intrinsics(K, f) or np.allclose(Kf, CA.scaled_intrinsics(K, f), rtol=1e-6)     # the binding starts from float32 K
        uf = np.stack([Kf[0] * c[:, 0] / c[:, 2] + Kf[2], Kf[1] * c[:, 1] / c[:, 2] + Kf[3]], 1)
        assert np.abs(uf * f + (f - 1) / 2.0 - u1).max() < 1e-9
    img = r.integers(0, 256, (9, 10, 3)).astype(np.uint8)
    assert (CM.box_filter(img, 1) == img).all() and CM.box_filter(img, 4).shape == (2, 2, 3) and CM.box_filter(img, 2).shape == (4, 5, 3)
    box = img[4:8, 4:8, 1].astype(int)
    assert int(CM.box_filter(img, 4)[1, 1, 1]) == (2 * box.sum() + 16) // 32
    assert int(CM.box_filter(np.array([[[1] * 3, [2] * 3], [[2] * 3, [1] * 3]], np.uint8), 2)[0, 0, 0]) == 2        # 1.5 rounds up


def test_statuses_of_the_mirror():
    """a constant image is SINGULAR, a single view has no targets and ends FEW, a held view stays FIXED"""
    sc = CM.scene(V=3, size=0.004, nx=20, ny=15)
    flat = [sc["colours"][0], np.full_like(sc["colours"][1], 77), sc["colours"][2]]
    rec = CM.run(sc["vertices"], sc["Rp"], sc["tp"], sc["K"], sc["rows"], sc["cols"], flat, fixed=(0,), rounds=2, iterations=2)["records"]
    assert list(rec["status"]) == [CM.FIXED, CM.SINGULAR, CM.RUNNING] and list(rec["iterations"]) == [0, 1, 4]
    assert rec["pose"][1].tobytes() == np.concatenate([sc["Rp"][1].reshape(9), sc["tp"][1]]).tobytes()
    rec = CM.run(sc["vertices"], sc["Rp"][1:2], sc["tp"][1:2], sc["K"], sc["rows"], sc["cols"], flat[2:], rounds=2, iterations=2)["records"]
    assert list(rec["status"]) == [CM.FEW] and rec["used"][0, 0] == 0 and rec["iterations"][0] == 1
    rec = CM.run(sc["vertices"], sc["Rp"], sc["tp"], sc["K"], sc["rows"], sc["cols"], sc["colours"], fixed=(0,), rounds=2, iterations=2, eps=1.0)["records"]
    assert list(rec["status"]) == [CM.FIXED, CM.CONVERGED, CM.CONVERGED] and list(rec["iterations"]) == [0, 2, 2]


# ---- the Python layer, the header and the library -----------------------------------------------------------------------------------------
def test_argument_checkers_refuse_what_the_header_refuses():
    assert CA.capacity_arg(1, 1) == (1, 1) and CA.capacity_arg(1 << 31, 2048) == (1 << 31, 2048)
    for v, w in ((0, 1), (1, 0), ((1 << 31) + 1, 1), (1, 2049), (1.0, 1), (1, True), (None, 1), (1, "1")):
        with pytest.raises(ValueError):
            CA.capacity_arg(v, w)
    assert CA.views_arg(1) == 1 and CA.views_arg(2048) == 2048 and CA.views_arg(3, 3) == 3
    for v, cap in ((0, 2048), (2049, 2048), (4, 3), (1.0, 2048), (None, 2048), (True, 2048)):
        with pytest.raises(ValueError):
            CA.views_arg(v, cap)
    assert CA.fixed_arg(None, 3) == () and CA.fixed_arg((2, 0), 3) == (0, 2) and CA.fixed_arg([], 3) == ()
    for v in ((3,), (-1,), (0, 0), 0, (0.0,), (True,), "0"):
        with pytest.raises(ValueError):
            CA.fixed_arg(v, 3)
    good = dict(huber=16.0, damping=0.0, eps=1e-7, min_pairs=6, min_views=2, rounds=4, iterations=3, stride=1)
    assert CA.rule_arg(**good) == (16.0, 0.0, 1e-7, 6, 2, 4, 3, 1)
    assert CA.rule_arg(**dict(good, rounds=256, iterations=1)) and CA.rule_arg(**dict(good, rounds=16, iterations=16))
    for name, values in (("huber", (0, -1.0, NAN, INF, 1e39, "x", None)), ("damping", (-1e-9, NAN, INF, "0", None, True)),
                         ("eps", (0, -1.0, NAN, INF, None, "1")), ("min_pairs", (5, 0, -1, 6.0, None, 1 << 32)),
                         ("min_views", (1, 0, 2.0, None, True)), ("rounds", (0, -1, 257, 1.0, None)), ("iterations", (0, 257, 1.0, None)),
                         ("stride", (0, -1, 1.0, None, 1 << 31))):
        for v in values:
            with pytest.raises(ValueError, match=name):
                CA.rule_arg(**dict(good, **{name: v}))
    with pytest.raises(ValueError, match="rounds \\* iterations"):
        CA.rule_arg(**dict(good, rounds=16, iterations=17))
    assert [CA.target_form_arg(f) for f in ("auto", "walk", "chunks")] == [0, 1, 2]
    for v in ("AUTO", 0, 1, None, "", b"walk"):
        with pytest.raises(ValueError):
            CA.target_form_arg(v)
    assert CA.scales_arg((4, 2, 1), 96, 128) == (4, 2, 1) and CA.scales_arg([1], 1, 1) == (1,)
    for v in ((), (0,), (17,), (2.0,), 4, (4,) * 9, (True,), None):
        with pytest.raises(ValueError):
            CA.scales_arg(v, 96, 128)
    with pytest.raises(ValueError):
        CA.scales_arg((4,), 3, 128)
    for K in ((1, 2, 3), (0, 1, 2, 3), (NAN, 1, 2, 3), "K"):
        with pytest.raises(ValueError):
            CA.scaled_intrinsics(K, 2)
    assert CA.scaled_intrinsics((140.0, 120.0, 63.5, 47.5), 2) == (70.0, 60.0, 31.5, 23.5)
    assert CA.MAX_VIEWS == CM.MAX_VIEWS and CA.MAX_ITERATIONS == CM.MAX_ITERATIONS and CA.STATUS == CM.STATUS_NAMES
    assert CA.RESULT == CM.RESULT_DTYPE and CA.RESULT.itemsize == 560
    assert ctypes.sizeof(CA.View) == 128 and ctypes.sizeof(CA.Rule) == 48 and CA.View.fixed.offset == ctypes.sizeof(RC.View) == 120


def test_the_header_is_valid_c(tmp_path):
    src = tmp_path / "colouralign.c"
    src.write_text('#include "rgbid_colouralign.h"\nint main(void) { rgbid_colouralign_view v; rgbid_colouralign_rule r; rgbid_colouralign_result q; '
                   '(void)v; (void)r; (void)q; return sizeof v == 128 && sizeof r == 48 && sizeof q == 560 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "colouralign")])
    assert subprocess.run([str(tmp_path / "colouralign")]).returncode == 0
    text = open(os.path.join(ROOT, "include", "rgbid_colouralign.h")).read()
    assert f"RGBID_COLOURALIGN_MAX_VIEWS {CA.MAX_VIEWS}" in text and f"RGBID_COLOURALIGN_MAX_ITERATIONS {CA.MAX_ITERATIONS}" in text
    assert f"RGBID_COLOURALIGN_MAX_FACTOR {CA.MAX_FACTOR}" in text and f"RGBID_COLOURALIGN_TERMS {CA.TERMS}" in text
    assert all(f"RGBID_COLOURALIGN_TARGET_{f.upper()} = {i}" in text for i, f in enumerate(CA.TARGET_FORMS))
    assert "RGBID_COLOURALIGN_FIXED = 4" in text and CA.FIXED == CM.FIXED == 4


def test_the_library_exports_the_colouralign_functions():
    from tests.test_abi import _declared
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared("rgbid_colouralign.h")
    assert set(names) == set(CA.EXPORTS) and len(names) == 7
    assert not [n for n in names if not hasattr(L, n)]
    L = _lib.bind(CA.SIGNATURES)
    h, ms = ctypes.c_void_p(), (ctypes.c_float * 3)()
    p, rule = RC.Params(0.05, 20.0, 0.02, 0.02, 0.2, 0), CA.Rule(16.0, 0.0, 1e-7, 6, 2, 1, 1, 1)
    assert L.rgbid_colouralign_create(None, None, 10, 2) == -1 and L.rgbid_colouralign_create(ctypes.byref(h), None, 10, 2) == -1 and not h.value
    assert L.rgbid_colouralign_run(None, None, None, 0, 1, None, None, 4, 4, ctypes.byref(p), ctypes.byref(rule), None) == -1
    assert L.rgbid_colouralign_targets(None, None, None, None) == -1 and L.rgbid_colouralign_timing(None, 0, ms) == -1
    assert L.rgbid_colouralign_downscale(None, None, 4, 4, 2, None) == -1 and L.rgbid_colouralign_destroy(None) == 0
    assert L.rgbid_colouralign_set_target_form(None, 0) == -1


def test_cli_option_errors(tmp_path):
    """every option error of the command line is raised before a device is touched"""
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    recolour = mesh_opt + ["--mesh-recolour", "mean"]
    for bad, word in ((mesh_opt + ["--mesh-colour-align"], "--mesh-colour-align needs --mesh-recolour or --mesh-texture"),
                      (recolour + ["--mesh-colour-align-rounds", "2"], "need --mesh-colour-align"),
                      (recolour + ["--mesh-colour-align", "--mesh-colour-align-scales", "2,x"], "--mesh-colour-align-scales: integers"),
                      (recolour + ["--mesh-colour-align", "--mesh-colour-align-rounds", "0"], "rounds")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()
