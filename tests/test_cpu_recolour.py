"""CPU checks of the recolouring stage (include/rgbid_recolour.h, rgbid.recolour): answers derived by hand; the numpy restatement the GPU
tests compare the kernels against (tests/recolour_mirror.py) against a scalar per-pair restatement written here; every class boundary
of the contract, exact in float32; the split of the views over calls; the Python argument checks one by one; the header as C99; the
library's exports and NULL-handle refusals."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from rgbid import _lib
from rgbid import recolour as RC
from tests import raster_mirror as XM
from tests import recolour_mirror as CM
from tests.render_mirror import pose_cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F, U8 = np.float32, np.uint8
EYE, ZERO = np.eye(3)[None], np.zeros((1, 3))
UNIT = (1.0, 1.0, 0.0, 0.0)              # with Z = 1 and the identity pose u = x and v = y exactly: a vertex is given in pixels
PARAMS = dict(z_min=0.5, z_max=4.0, surface_tolerance=0.25, measured_tolerance=0.25, min_cos=0.2, two_sided=False)
OPTIONAL = ("normals", "surface", "depthinv")


def case(vertices, colours, K=UNIT, R=EYE, t=ZERO, normals=None, surface=None, depthinv=None, **params):
    """colours: [V, rows, cols, 3]; surface, depthinv: [V, rows, cols] or None"""
    col = np.ascontiguousarray(colours, U8)
    V, rows, cols = col.shape[:3]
    R, t = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3)
    if len(R) == 1 and V > 1:
        R, t = np.repeat(R, V, 0), np.repeat(t, V, 0)
    plane = lambda x: None if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, F), (V, rows, cols)))
    return dict(vertices=np.array(vertices, F).reshape(-1, 3), normals=None if normals is None else np.array(normals, F).reshape(-1, 3), R=R, t=t,
                K=K, rows=rows, cols=cols, colours=col, surface=plane(surface), depthinv=plane(depthinv), params=dict(PARAMS, **params))


def mirror(c, mode="mean", split=None, colours_in=None, drop=()):
    """the mirror's result of a case, without the optional inputs named in `drop`"""
    opt = {k: None if k in drop else c[k] for k in OPTIONAL}
    return CM.recolour_numpy(c["vertices"], c["R"], c["t"], c["K"], c["rows"], c["cols"], c["colours"], mode, colours_in, split, **opt, **c["params"])


def constant(colour, rows=4, cols=4):
    return np.broadcast_to(np.array(colour, U8), (rows, cols, 3))


def classes(c, **kw):
    """the class of every (view, vertex) pair, from the per-view counts of one-vertex runs"""
    out = []
    for i in range(len(c["vertices"])):
        one = dict(c, vertices=c["vertices"][i:i + 1], normals=None if c["normals"] is None else c["normals"][i:i + 1])
        cnt = mirror(one, **kw)["counts"]
        assert (cnt.sum(1) == 1).all()
        out.append([CM.COUNTS[int(np.argmax(row))] for row in cnt])
    return np.array(out).T.tolist()      # [view][vertex]


# ---- answers derived by hand ------------------------------------------------------------------------------------------------------------
def test_one_vertex_over_four_colours():
    """u = 0.25, v = 0.75: xs = 64, ys = 192, so the weights are 192 * 64, 64 * 64, 192 * 192, 64 * 192 = 12288 4096 36864 12288 of 65536"""
    img = np.array([[(10, 20, 30), (110, 120, 130)], [(50, 60, 70), (250, 240, 230)]], U8)[None]
    c = case([(0.25, 0.75, 1.0)], img)
    s = [12288 * 10 + 4096 * 110 + 36864 * 50 + 12288 * 250, 12288 * 20 + 4096 * 120 + 36864 * 60 + 12288 * 240,
         12288 * 30 + 4096 * 130 + 36864 * 70 + 12288 * 230]
    assert s == [5488640, 5898240, 6307840]                                      # / 65536 = 83.75, 90.0, 96.25
    for mode in ("mean", "best"):
        out = mirror(c, mode)
        assert out["colours"].tolist() == [[84, 90, 96]] and out["views_used"].tolist() == [1] and out["counts"].tolist() == [[0, 0, 0, 0, 0, 1]]
        state = np.frombuffer(out["state"][:32], np.uint64)
        assert state.tolist() == ([1024 * x for x in s] + [1024] if mode == "mean" else s + [(1024 << 32) | 0xFFFFFFFF])
    assert mirror(c, "best")["best_view"].tolist() == [0]


def test_a_constant_image_gives_its_colour():
    rng = np.random.default_rng(3)
    pts = [(x, y, 1.0) for x, y in rng.uniform(0, 3, (40, 2))]
    for colour in ((0, 0, 0), (255, 255, 255), (1, 128, 254)):
        c = case(pts, constant(colour)[None])
        for mode in ("mean", "best"):
            out = mirror(c, mode)
            assert (out["colours"] == np.array(colour, U8)).all() and (out["views_used"] == 1).all()


def test_a_column_ramp_rounds_as_derived():
    """c = 10 px in a 1 x 8 image: xs = 640, 652, 653 and 589 give 20 + 10 ax / 256 = 25.0, 25.47, 25.51 and 23.008"""
    img = np.repeat((10 * np.arange(8, dtype=U8))[None, :, None], 3, 2)[None]
    c = case([(2.5, 0, 1), (652 / 256, 0, 1), (2.55, 0, 1), (2.3, 0, 1), (7, 0, 1), (0, 0, 1)], img)
    for mode in ("mean", "best"):
        assert mirror(c, mode)["colours"][:, 0].tolist() == [25, 25, 26, 23, 70, 0]


def two_view_case(second=42):
    """a vertex with the normal 0 0 -1 seen head-on (cos = 1, w = 1024) by view 0 and from 60 degrees (cos = 0.5, w = 512) by view 1"""
    a = math.radians(60.0)
    R1 = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    p = np.array([0.0, 0.0, 1.0])
    t1 = p - R1 @ np.array([0.0, 0.0, 1.0])                  # the vertex lies at 0 0 1 of view 1 as well
    img = np.stack([constant((100, 100, 100), 5, 5), constant((second,) * 3, 5, 5)])
    return case([p], img, K=(1.0, 1.0, 2.0, 2.0), R=np.stack([np.eye(3), R1]), t=np.stack([np.zeros(3), t1]), normals=[(0, 0, -1)])


def test_weights_1024_and_512_give_the_derived_mean():
    c = two_view_case()
    out = mirror(c)
    assert np.frombuffer(out["state"][24:32], np.uint64)[0] == 1536 and out["views_used"].tolist() == [2]
    assert out["colours"].tolist() == [[81] * 3]             # (1024 * 100 + 512 * 42) / 1536 = 80.67
    assert mirror(two_view_case(41))["colours"].tolist() == [[80] * 3]           # 80.33
    best = mirror(c, "best")
    assert best["colours"].tolist() == [[100] * 3] and best["best_view"].tolist() == [0]
    swapped = dict(c, R=c["R"][::-1], t=c["t"][::-1], colours=c["colours"][::-1])
    best = mirror(swapped, "best")
    assert best["colours"].tolist() == [[100] * 3] and best["best_view"].tolist() == [1]     # the larger weight wins, wherever it stands


def test_best_ties_go_to_the_earlier_view():
    img = np.stack([constant((10, 20, 30)), constant((200, 210, 220)), constant((90, 90, 90))])
    c = case([(1.5, 1.5, 1.0), (NAN, 0, 1)], img)
    out = mirror(c, "best", colours_in=np.array([(1, 2, 3), (4, 5, 6)], U8))
    assert out["colours"].tolist() == [[10, 20, 30], [4, 5, 6]] and out["best_view"].tolist() == [0, 0xFFFFFFFF] and out["views_used"].tolist() == [3, 0]
    assert mirror(c, "best")["colours"].tolist() == [[10, 20, 30], [0, 0, 0]]
    assert mirror(c, "mean")["colours"].tolist() == [[100, 107, 113], [0, 0, 0]]            # 300 / 3, 320 / 3 = 106.67, 340 / 3 = 113.33


# ---- the scalar restatement: one (vertex, view) pair at a time, Python integers and floats ------------------------------------------------
def pair_loop(p, n, m, K, rows, cols, colour, surface, measured, z_min, z_max, surface_tolerance, measured_tolerance, min_cos, two_sided):
    """-> (class name, w, [s_0, s_1, s_2]) of one pair; w and s only when it is taken"""
    rec = XM.project_loop(p, m, K, z_min, z_max)
    if rec is None:
        return "gated", None, None
    xs, ys, Z = rec
    if not (0 <= xs <= 256 * (cols - 1) and 0 <= ys <= 256 * (rows - 1)):
        return "outside", None, None
    x0, ax, y0, ay = xs >> 8, xs & 255, ys >> 8, ys & 255
    x1, y1 = min(x0 + 1, cols - 1), min(y0 + 1, rows - 1)
    foot = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    with np.errstate(all="ignore"):
        if surface is not None:
            for at in foot:
                d = F(surface[at])
                if not math.isfinite(float(d)) or abs(F(Z - d)) > F(surface_tolerance):
                    return "hidden", None, None
        if measured is not None:
            for at in foot:
                iD = F(measured[at])
                if not math.isfinite(float(iD)) or not iD > 0:
                    return "unmeasured", None, None
                z = F(F(1) / iD)
                if not math.isfinite(float(z)) or abs(F(Z - z)) > F(measured_tolerance):
                    return "unmeasured", None, None
        w = 1024
        if n is not None:
            n0, n1, n2 = (F(v) for v in n)
            q = F(F(F(n0 * n0) + F(n1 * n1)) + F(n2 * n2))
            if math.isfinite(float(q)) and q != 0:
                x, y, z = (F(v) for v in p)
                X = F(F(F(F(m[0] * x) + F(m[1] * y)) + F(m[2] * z)) + m[9])
                Y = F(F(F(F(m[3] * x) + F(m[4] * y)) + F(m[5] * z)) + m[10])
                c = [float(F(F(F(m[3 * k] * n0) + F(m[3 * k + 1] * n1)) + F(m[3 * k + 2] * n2))) for k in range(3)]
                Xd, Yd, Zd = float(X), float(Y), float(Z)
                dot = -((c[0] * Xd + c[1] * Yd) + c[2] * Zd)
                g = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                r = (Xd * Xd + Yd * Yd) + Zd * Zd
                cos = float(np.float64(dot) / np.sqrt(np.float64(g) * np.float64(r)))      # numpy: 0 / 0 and inf / inf are NaN, not errors
                if two_sided:
                    cos = abs(cos)
                if not (cos > 0 and cos >= float(F(min_cos))):
                    return "averted", None, None
                w = max(1, math.floor(cos * 1024.0 + 0.5))
    wt = [(256 - ax) * (256 - ay), ax * (256 - ay), (256 - ax) * ay, ax * ay]
    return "taken", w, [sum(wt[j] * int(colour[foot[j]][k]) for j in range(4)) for k in range(3)]


def recolour_loop(c, mode="mean", colours_in=None, drop=()):
    """the whole contract as loops over the pairs -> dict(colours, views_used, best_view, counts)"""
    opt = {k: None if k in drop else c[k] for k in OPTIONAL}
    n_v, V = len(c["vertices"]), len(c["R"])
    counts = np.zeros((V, 6), np.int64)
    out = dict(colours=np.zeros((n_v, 3), U8), views_used=np.zeros(n_v, np.uint32), best_view=np.full(n_v, 0xFFFFFFFF, np.uint32), counts=counts)
    ms = [pose_cw(c["R"][v], c["t"][v]) for v in range(V)]
    for i in range(n_v):
        S, W, used, best = [0, 0, 0], 0, 0, None
        for v in range(V):
            cls, w, s = pair_loop(c["vertices"][i], None if opt["normals"] is None else opt["normals"][i], ms[v], c["K"], c["rows"], c["cols"],
                                  c["colours"][v], None if opt["surface"] is None else opt["surface"][v],
                                  None if opt["depthinv"] is None else opt["depthinv"][v], **c["params"])
            counts[v, CM.COUNTS.index(cls)] += 1
            if cls != "taken":
                continue
            used += 1
            S, W = [a + w * b for a, b in zip(S, s)], W + w
            if best is None or w > best[0]:
                best = (w, v, s)
        out["views_used"][i] = used
        if not used:
            out["colours"][i] = 0 if colours_in is None else colours_in[i]
        elif mode == "mean":
            out["colours"][i] = [(2 * a + 65536 * W) // (2 * 65536 * W) for a in S]
        else:
            out["colours"][i] = [(a + 32768) >> 16 for a in best[2]]
            out["best_view"][i] = best[1]
    if mode != "best":
        del out["best_view"]
    return out


def random_case(n_v, V, rows=12, cols=16, seed=0, bad=0.04):
    """n_v vertices around the plane Z = 2 in front of V cameras near the origin, smooth surface and inverse-depth planes near that depth
    with NaN, infinite, zero and negative entries, random images, normals of every length; a share `bad` of the coordinates, normals and
    texels is not finite or otherwise unusable"""
    rng = np.random.default_rng(seed)
    K = (0.9 * cols, 0.9 * cols, (cols - 1) / 2, (rows - 1) / 2)
    pos = np.stack([rng.uniform(-1.6, 1.6, n_v), rng.uniform(-1.3, 1.3, n_v), rng.normal(2.0, 0.35, n_v)], 1).astype(F)
    nrm = rng.normal(size=(n_v, 3)) * np.array([0.6, 0.6, 1.0])
    nrm[:, 2] = -np.abs(nrm[:, 2]) * np.where(rng.random(n_v) < 0.8, 1, -1)
    nrm = (nrm * 10.0 ** rng.uniform(-3, 3, (n_v, 1))).astype(F)
    pick = lambda shape: rng.random(shape) < bad
    poison = np.array([NAN, INF, -INF], F)
    pos = np.where(pick(pos.shape) & (rng.random(pos.shape) < 0.5), rng.choice(poison, pos.shape), pos).astype(F)
    nrm[pick(n_v)] = 0
    nrm = np.where(pick(nrm.shape) & (rng.random(nrm.shape) < 0.3), rng.choice(poison, nrm.shape), nrm).astype(F)
    R, t = [], []
    for v in range(V):
        w = rng.normal(0, 0.12, 3)
        a = np.linalg.norm(w)
        k = w / a
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R.append(np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx)
        t.append(rng.normal(0, 0.15, 3))
    yy, xx = np.mgrid[0:rows, 0:cols]
    wave = lambda: 2.0 + 0.45 * np.sin(xx / cols * rng.uniform(2, 5) + rng.uniform(0, 6)) * np.cos(yy / rows * rng.uniform(2, 5) + rng.uniform(0, 6))
    surface = np.stack([wave() for _ in range(V)]).astype(F)
    depthinv = (1.0 / np.stack([wave() for _ in range(V)])).astype(F)
    surface = np.where(pick(surface.shape), rng.choice(np.array([NAN, INF, -INF, 0.0, -2.0], F), surface.shape), surface).astype(F)
    depthinv = np.where(pick(depthinv.shape), rng.choice(np.array([NAN, INF, -INF, 0.0, -0.5, 1e-42], F), depthinv.shape), depthinv).astype(F)
    colours = rng.integers(0, 256, (V, rows, cols, 3)).astype(U8)
    return case(pos, colours, K, np.stack(R), np.stack(t), nrm, surface, depthinv, z_min=1.6, z_max=2.6, surface_tolerance=0.3, measured_tolerance=0.3,
                min_cos=0.3, two_sided=bool(seed & 1))


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in b)


@pytest.mark.parametrize("mode", ["mean", "best"])
@pytest.mark.parametrize("drop", [(), ("normals",), ("surface",), ("depthinv",), ("surface", "depthinv"), OPTIONAL])
def test_mirror_against_the_scalar_restatement(mode, drop):
    seen = np.zeros(6, np.int64)
    for seed in range(4):
        c = random_case(60 - seed, 3, seed=seed + 10 * len(drop))
        cin = np.random.default_rng(seed).integers(0, 256, (len(c["vertices"]), 3)).astype(U8) if seed & 2 else None
        got, want = mirror(c, mode, colours_in=cin, drop=drop), recolour_loop(c, mode, cin, drop)
        assert same(got, want), (seed, got["counts"], want["counts"])
        assert (got["counts"].sum(1) == len(c["vertices"])).all()
        seen += got["counts"].sum(0)
    assert seen[0] and seen[1] and seen[5] and (("surface" in drop) or seen[2]) and (("depthinv" in drop) or seen[3]) and (("normals" in drop) or seen[4])


# ---- class boundaries ------------------------------------------------------------------------------------------------------------------
def up(x):
    return float(np.nextafter(F(x), F(INF)))


def down(x):
    return float(np.nextafter(F(x), F(-INF)))


def boundary_cases():
    """name -> (case, the class of every pair [view][vertex]); everything exact in float32"""
    img = np.random.default_rng(1).integers(0, 256, (1, 3, 5, 3)).astype(U8)
    out = {}
    out["depth_gate"] = (case([(0, 0, 0.5), (0, 0, down(0.5)), (0, 0, 4.0), (0, 0, up(4.0))], img), [["taken", "gated", "taken", "gated"]])
    s = 1 / 256
    out["image_edges"] = (case([(0, 0, 1), (-s, 0, 1), (0, -s, 1), (4, 2, 1), (4 + s, 2, 1), (4, 2 + s, 1), (4 - s, 2 - s, 1), (-0.5 * s, 0, 1), (-0.51 * s, 0, 1)], img),
                          [["taken", "outside", "outside", "taken", "outside", "outside", "taken", "taken", "outside"]])
    out["one_by_one"] = (case([(0, 0, 1), (s, 0, 1), (0, 0.4 * s, 1), (0, 0, NAN), (INF, 0, 1), (0, -INF, 1)], img[:, :1, :1]),
                         [["taken", "outside", "taken", "gated", "gated", "gated"]])
    out["one_row"] = (case([(0, 0, 1), (3.5, 0, 1), (4, 0, 1), (4, s, 1)], img[:, :1]), [["taken", "taken", "taken", "outside"]])
    near = np.full((3, 5), 1.25, F)
    far = near.copy(); far[1, 2] = up(1.25)
    pts = [(1.5, 0.5, 1), (0.5, 0.5, 1), (3, 1, 1), (2, 1, 1)]                      # the first and the last footprint hold texel (2, 1)
    out["surface_at_the_tolerance"] = (case(pts, img, surface=near), [["taken"] * 4])
    out["surface_one_ulp_beyond"] = (case(pts, img, surface=far), [["hidden", "taken", "taken", "hidden"]])
    out["surface_tolerance_one_ulp_less"] = (case(pts, img, surface=near, surface_tolerance=down(0.25)), [["hidden"] * 4])
    out["surface_tolerance_zero"] = (case(pts, img, surface=np.ones((3, 5), F), surface_tolerance=0.0), [["taken"] * 4])
    holes = np.ones((3, 5), F); holes[0, 0] = NAN; holes[2, 4] = INF; holes[0, 4] = -INF
    out["surface_holes"] = (case([(0.5, 0.5, 1), (1, 1, 1), (3.5, 1.5, 1), (2, 0, 1), (3, 0, 1), (2, 1.5, 1)], img, surface=holes),
                            [["hidden", "taken", "hidden", "taken", "hidden", "taken"]])     # (3, 0): the hole at (4, 0) has weight 0 and still hides
    for name, m, cls in (("zero", 0.0, "unmeasured"), ("negative", -1.0, "unmeasured"), ("denormal", 1e-42, "unmeasured"), ("infinite", INF, "unmeasured"),
                         ("nan", NAN, "unmeasured"), ("at_the_tolerance", 0.8, "taken"), ("beyond", down(0.8), "unmeasured"), ("small", 2e-38, "unmeasured")):
        plane = np.ones((3, 5), F); plane[1, 2] = m
        out["measured_" + name] = (case(pts, img, depthinv=plane), [[cls, "taken", "taken", cls]])
    both = np.ones((3, 5), F); both[1, 2] = NAN
    out["hidden_before_unmeasured"] = (case(pts, img, surface=both, depthinv=both), [["hidden", "taken", "taken", "hidden"]])
    nr = [(0, 0, -1), (0, 3, -4), (0, 0, 1), (0, 0, 0), (NAN, 0, 1), (0, INF, 1), (0, 4, -3), (1e-30, 0, 1e-30), (1e20, 0, 1e20)]
    mid = [(0, 0, 1)] * len(nr)
    out["facing"] = (case(mid, img, normals=nr, min_cos=0.75), [["taken", "taken", "averted", "taken", "taken", "taken", "averted", "taken", "taken"]])
    out["facing_min_cos_one"] = (case(mid, img, normals=nr, min_cos=1.0), [["taken", "averted", "averted", "taken", "taken", "taken", "averted", "taken", "taken"]])
    out["facing_min_cos_above"] = (case(mid, img, normals=nr, min_cos=0.8), [["taken", "averted", "averted", "taken", "taken", "taken", "averted", "taken", "taken"]])
    out["facing_two_sided"] = (case(mid, img, normals=nr, min_cos=0.75, two_sided=True), [["taken", "taken", "taken", "taken", "taken", "taken", "averted", "taken", "taken"]])
    out["facing_edge_on"] = (case(mid[:2], img, normals=[(1, 0, 0), (0, -2, 0)], min_cos=0.0, two_sided=True), [["averted", "averted"]])
    return out


BOUNDARIES = boundary_cases()


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_class_boundaries(name):
    c, want = BOUNDARIES[name]
    assert classes(c) == want
    for mode in ("mean", "best"):
        assert same(mirror(c, mode), recolour_loop(c, mode))


def test_boundary_weights():
    """cos = 4 / 5 gives w = floor(819.2 + 0.5) = 819; squared lengths that underflow to 0 or overflow in float32 skip the test: w = 1024"""
    c, _ = BOUNDARIES["facing"]
    c = dict(c, colours=np.ascontiguousarray(constant((255, 255, 255), 3, 5)[None]))
    W = np.frombuffer(mirror(c)["state"][:32 * 9], np.uint64)[3 * 9:4 * 9]
    assert W.tolist() == [1024, 819, 0, 1024, 1024, 1024, 0, 1024, 1024]
    grazing = case([(0, 0, 1)], c["colours"], normals=[(1, 0, -1e-5)], min_cos=0.0)
    assert np.frombuffer(mirror(grazing)["state"][:32], np.uint64)[3] == 1       # cos = 1e-5: floor(0.51) = 0, raised to 1


def test_the_split_of_the_views_changes_nothing():
    c = random_case(50, 17, seed=5)
    for mode in ("mean", "best"):
        whole = mirror(c, mode)
        for split in (16, 1):
            part = mirror(c, mode, split=split)
            assert part["state"] == whole["state"] and same(part, whole) and len(part["counts"]) == 17


# ---- the Python layer, the header and the library -----------------------------------------------------------------------------------------
def test_argument_checkers_refuse_what_the_header_refuses():
    for f, good, bad in ((RC.capacity_arg, (1, 1 << 31, np.int64(5)), (0, -1, (1 << 31) + 1, 1.0, True, "1", None)),
                         (RC.count_arg, (0, 1, 1 << 31), (-1, (1 << 31) + 1, 0.0, False, None)),
                         (RC.mode_arg, ("mean", "best"), ("MEAN", 0, 1, None, "", b"mean")),
                         (RC.cos_arg, (0, 1, 0.2, np.float32(0.5)), (-1e-6, 1.0001, NAN, INF, "0.2", None, True)),
                         (RC.batch_arg, (1, 16, 4096), (0, 4097, 1.0, None)),
                         (RC.views_arg, (1, 65535), (0, -1, 65536, 1.0, None, True))):
        for v in good:
            f(v)
        for v in bad:
            with pytest.raises(ValueError):
                f(v)
    assert RC.mode_arg("mean") == 0 and RC.mode_arg("best") == 1
    assert RC.views_arg(1, 65534) == 1
    with pytest.raises(ValueError):
        RC.views_arg(2, 65534)
    with pytest.raises(ValueError):
        RC.count_arg(11, 10)
    for v in (0, 0.0, 0.02, 1e30, np.float32(1)):
        RC.tolerance_arg("surface_tolerance", v)
    for v in (-1e-9, NAN, INF, -INF, 1e39, "0.02", None, True):
        with pytest.raises(ValueError, match="measured_tolerance"):
            RC.tolerance_arg("measured_tolerance", v)
    for v in (True, False, 0, 1, np.bool_(True)):
        assert RC.flag_arg("two_sided", v) in (0, 1)
    for v in (2, -1, 1.0, "yes", None):
        with pytest.raises(ValueError):
            RC.flag_arg("two_sided", v)
    assert RC.image_size(1, 16384) == (1, 16384)
    for rows, cols in ((0, 4), (4, 0), (16385, 4), (4, 16385), (4.0, 4), (None, 4)):
        with pytest.raises(ValueError):
            RC.image_size(rows, cols)
    import torch
    host = torch.zeros((4, 3))
    for f, args in ((RC.vertices_arg, (host,)), (RC.vertices_arg, (np.zeros((4, 3), F),)), (RC.colour_planes_arg, (torch.zeros((1, 2, 2, 3), dtype=torch.uint8), 1, 2, 2)),
                    (RC.colour_planes_arg, (None, 1, 2, 2)), (RC.colour_planes_arg, ([], 1, 2, 2)), (RC.depth_planes_arg, ("surface", torch.zeros((1, 2, 2)), 1, 2, 2)),
                    (RC.depth_planes_arg, ("depthinv", [None, None], 1, 2, 2)), (RC.depth_planes_arg, ("depthinv", 5, 1, 2, 2)),
                    (RC.output_arg, ("views_used", torch.zeros(4, dtype=torch.int32), RC.A.int4, (4,))),
                    (RC.keyframes_arg, ([], False)), (RC.keyframes_arg, ([dict(R=0, t=0)], False)), (RC.keyframes_arg, ([dict(R=0, t=0, colour=1)], True))):
        with pytest.raises(ValueError):
            f(*args)
    assert RC.depth_planes_arg("surface", None, 3, 2, 2) == [None] * 3 and RC.output_arg("best_view", None, RC.A.int4, (4,)) is None
    assert RC.keyframes_arg([dict(R=0, t=0, colour=1)], False)
    assert ctypes.sizeof(RC.Params) == 24 and ctypes.sizeof(RC.View) == 120


def test_the_header_is_valid_c(tmp_path):
    src = tmp_path / "recolour.c"
    src.write_text('#include "rgbid_recolour.h"\nint main(void) { rgbid_recolour_params p; rgbid_recolour_view v; (void)p; (void)v; '
                   'return sizeof p == 24 && sizeof v == 120 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "recolour")])
    assert subprocess.run([str(tmp_path / "recolour")]).returncode == 0
    text = open(os.path.join(ROOT, "include", "rgbid_recolour.h")).read()
    assert f"RGBID_RECOLOUR_MAX_VIEWS {RC.MAX_VIEWS}" in text and f"RGBID_RECOLOUR_VIEW_CHUNK {RC.VIEW_CHUNK}" in text
    assert f"RGBID_RECOLOUR_UNIT_WEIGHT {RC.UNIT_WEIGHT}" in text and CM.MAX_VIEWS == RC.MAX_VIEWS and CM.UNIT == RC.UNIT_WEIGHT


def test_the_library_exports_the_recolour_functions():
    from tests.test_abi import _declared
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared("rgbid_recolour.h")
    assert set(names) == set(RC.EXPORTS) and len(names) == 7
    assert not [n for n in names if not hasattr(L, n)]
    L = _lib.bind(RC.SIGNATURES)
    h, out, ms = ctypes.c_void_p(), (ctypes.c_ulonglong * 6)(), (ctypes.c_float * 2)()
    p = RC.Params(0.05, 20.0, 0.02, 0.02, 0.2, 0)
    assert L.rgbid_recolour_create(None, None, 10) == -1 and L.rgbid_recolour_create(ctypes.byref(h), None, 10) == -1 and not h.value
    assert L.rgbid_recolour_begin(None, 0, 0) == -1 and L.rgbid_recolour_finish(None, None, None, None, None) == -1
    assert L.rgbid_recolour_add(None, None, None, 0, 1, None, None, 4, 4, ctypes.byref(p)) == -1
    assert L.rgbid_recolour_counts(None, 0, 1, out) == -1 and L.rgbid_recolour_timing(None, 0, ms) == -1 and L.rgbid_recolour_destroy(None) == 0
