"""CPU checks of the registration stage (include/rgbid_meshreg.h, rgbid.meshreg): the vectorised numpy restatement the GPU tests compare
the kernels against (tests/meshreg_mirror.py) against its scalar loops; every threshold of the contract on the mirror; an input whose sum
depends on the order; convergence on section 18's surface and the choice among the four principal starts on a surface without its
symmetry; `choose` by hand; the Python argument checks one by one; the header as C99; the library's exports and NULL-handle refusals; the
command lines' option errors."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import _lib
from rgbid import meshreg as MR
from tests import align_mirror as AM
from tests import meshreg_mirror as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
IDENTITY = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
PLANE_V = [(-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0)]         # a flat target of two triangles at z = 0
PLANE_T = [(0, 1, 2), (0, 2, 3)]
# what the mirror reaches on the prototype scene on the CPU: the tessellation's chord error, not the method's
MIRROR_ROTATION, MIRROR_TRANSLATION, MIRROR_RMS = 6.25e-4, 8.5e-4, 1.41e-4


def up(x, towards=INF):
    return np.nextafter(F(x), F(towards))


def pose_of(R, t):
    return np.concatenate([np.asarray(R, D).reshape(9), np.asarray(t, D).reshape(3)])


# ---- the scenes the GPU tests share ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prototype(asymmetric=False):
    """the prototype scene: the height field of 33 x 25 vertices, d_max 0.4 m, and 600 analytic points -> (Target, points float32)"""
    v, t = RM.height_field(asymmetric=asymmetric)
    return RM.Target(v, t, 0.4), RM.surface_points(asymmetric=asymmetric).astype(F)


@functools.lru_cache(maxsize=None)
def small_scene():
    """a coarse height field (96 triangles) and 70 points: small enough for the scalar loops"""
    v, t = RM.height_field(9, 7)
    return RM.Target(v, t, 0.4), RM.surface_points(70, seed=11).astype(F)


def perturbed_starts(n, angle, shift, seed=100):
    P = [RM.perturbation(seed + s, angle, shift) for s in range(n)]
    return np.stack([p[0] for p in P]), np.stack([p[1] for p in P])


def plane_target(d_max=0.5):
    return RM.Target(np.array(PLANE_V, F), np.array(PLANE_T), d_max)


# ---- the two restatements -------------------------------------------------------------------------------------------------------------------
def test_mirror_equals_the_loops():
    tg, pts = small_scene()
    R, t = perturbed_starts(2, 0.04, 0.05)
    kw = dict(levels=((2, 2, 0.4), (1, 1, 0.2)), huber=0.004, damping=1e-3, eps=1e-7, min_points=6)
    pv = RM.point_values(tg, RM.transform(pose_of(R[0], t[0]), pts), 0.4, kw["huber"])
    w = pv["w"][pv["used"]]
    assert (w == 1).any() and (w < 1).any(), "both weight branches occur"
    a, b = RM.align(tg, pts, R, t, **kw), RM.align_loop(tg, pts, R, t, **kw)
    assert a.tobytes() == b.tobytes()
    assert (a["iterations"] == 3).all() and (a["used"] > 6).all() and (a["used"][:, 0] < a["used"][:, 1]).all()
    n, has = RM.normals(tg.v, tg.t)
    for k in range(len(tg.t)):
        one = RM._normal_loop(tg.v, tg.t[k])
        assert has[k] and np.array(one, D).tobytes() == n[k].tobytes()
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-15 and (n[:, 2] > 0).all()


# ---- thresholds, each on the mirror ---------------------------------------------------------------------------------------------------------
def test_reach_to_the_ulp():
    tg = plane_target()
    for z, reach, used in ((0.125, 0.125, 1), (up(0.125), 0.125, 0), (0.125, up(0.125, 0), 0), (-0.125, 0.125, 1), (up(0.125), up(0.125), 1)):
        n, sums = RM.system(tg, np.array([(0.3, 0.2, z)], F), IDENTITY, 1, reach, 0.5)
        assert n == used and (sums[0] == 0) and (sums[27] > 0) == bool(used), (z, reach)


def test_huber_to_the_ulp():
    tg = plane_target()
    for z, huber, w in ((0.125, 0.125, 1.0), (up(0.125), 0.125, 0.125 / float(up(0.125))), (0.125, up(0.125, 0), float(up(0.125, 0)) / 0.125)):
        p = np.array([(0.3, 0.2, z)], F)
        pv = RM.point_values(tg, p, 0.5, huber)
        assert pv["used"][0] and pv["f"][0] == float(F(z)) and pv["w"][0] == w and (w == 1.0) == (float(F(z)) <= float(F(huber)))
        n, sums = RM.system(tg, p, IDENTITY, 1, 0.5, huber)
        assert n == 1 and sums[27] == (w * float(F(z))) * float(F(z)) and sums[11] == w        # a_2 J_2 = w n2 n2


def test_degenerate_winners_are_not_used():
    v = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0.5, 0.5, 0.5)], F)
    for tri in ([(3, 3, 3)], [(0, 1, 2)], [(0, 2, 1)]):                                      # zero area: a point; three collinear corners, both ways
        tg = RM.Target(v, np.array(tri), 1.0)
        assert not tg.has.any() and np.isnan(tg.normals).all() and tg.normals.view(np.uint64).tolist() == [[int(AM.NAN_BITS)] * 3]
        pv = RM.point_values(tg, np.array([(0.5, 0.4, 0.4)], F), 1.0, 0.5)
        assert pv["triangle"][0] == 0 and pv["distance"][0] < 1.0 and not pv["used"][0]
        n, sums = RM.system(tg, np.array([(0.5, 0.4, 0.4)], F), IDENTITY, 1, 1.0, 0.5)
        assert n == 0 and sums.tobytes() == np.zeros(28).tobytes()
    # a triangle with a non-finite corner takes no part; its neighbour still answers
    v = np.array(PLANE_V + [(0, 0, NAN)], F)
    tg = RM.Target(v, np.array(PLANE_T + [(0, 1, 4)]), 0.5)
    assert tg.has.tolist() == [True, True, False] and RM.system(tg, np.array([(0.3, 0.2, 0.1)], F), IDENTITY, 1, 0.5, 0.5)[0] == 1


def test_non_finite_points_are_not_used():
    tg, pts = small_scene()
    bad = pts.copy()
    bad[[3, 17, 40]] = [(NAN, 0, 1.8), (0, INF, 1.8), (0, 0, -INF)]
    n0, s0 = RM.system(tg, pts, IDENTITY, 1, 0.4, 0.4)
    n1, s1 = RM.system(tg, bad, IDENTITY, 1, 0.4, 0.4)
    assert n0 == 70 and n1 == 67 and np.isfinite(s1).all()
    keep = np.ones(70, bool); keep[[3, 17, 40]] = False
    zeroed = np.where(keep[None], RM.terms_of(RM.point_values(tg, pts, 0.4, 0.4)), 0.0)
    assert AM.reduce_tiles(AM.tree64(RM.group_lanes(zeroed))).tobytes() == s1.tobytes()
    huge = RM.transform(pose_of(np.eye(3) * 3e38, (0, 0, 0)), pts[:4])                      # a finite pose whose float32 point overflows
    assert np.isinf(huge).any() and RM.system(tg, pts[:4], pose_of(np.eye(3) * 3e38, (0, 0, 0)), 1, 0.4, 0.4)[0] == 0


def test_min_points_to_the_point():
    tg, pts = small_scene()
    R, t = perturbed_starts(1, 0.01, 0.01)
    six = pts[:6]
    ok = RM.align(tg, six, R, t, levels=((1, 2, 0.4),), min_points=6)
    few = RM.align(tg, six, R, t, levels=((1, 2, 0.4),), min_points=7)
    assert ok["used"].tolist() == [[6, 6]] and ok["status"][0] != RM.FEW and ok["iterations"][0] == 2
    assert few["status"][0] == RM.FEW and few["iterations"][0] == 1 and few["used"].tolist() == [[6, 6]]
    assert few["pose"][0].tobytes() == pose_of(R[0], t[0]).tobytes() and ok["pose"][0].tobytes() != few["pose"][0].tobytes()
    assert few["sums"][0, 0].tobytes() == few["sums"][0, 1].tobytes() == ok["sums"][0, 0].tobytes()


def test_a_flat_target_is_singular():
    tg = plane_target()
    r = np.random.default_rng(4)
    pts = np.c_[r.uniform(-1, 1, (40, 2)), np.full(40, 0.01)].astype(F)
    R, t = perturbed_starts(1, 0.01, 0.01, seed=7)
    t[0] = (0.01, -0.02, 0.03)
    res = RM.align(tg, pts, R, t, levels=((1, 3, 0.5),))
    assert res["status"][0] == RM.SINGULAR and res["iterations"][0] == 1 and res["used"].tolist() == [[40, 40]]
    assert res["pose"][0].tobytes() == pose_of(R[0], t[0]).tobytes()
    assert res["sums"][0, 0, 0] == 0 and res["sums"][0, 0, 11] == 40                          # no normal has an x component; sum of n2 n2
    damped = RM.align(tg, pts, R, t, levels=((1, 3, 0.5),), damping=1e-3)                   # the damping scales the diagonal: a zero stays zero
    assert damped["status"][0] == RM.SINGULAR


def test_levels_restart_converged_starts_and_leave_few_ones():
    tg, pts = prototype()
    R, t = perturbed_starts(1, 0.01, 0.01)
    R = np.concatenate([R, np.eye(3)[None]]); t = np.concatenate([t, [(0, 0, 5.0)]])
    first = RM.align(tg, pts, R, t, levels=((4, 12, 0.4),), eps=1e-4)
    both = RM.align(tg, pts, R, t, levels=((4, 12, 0.4), (2, 12, 0.2)), eps=1e-4)
    assert first["status"].tolist() == [RM.CONVERGED, RM.FEW] and both["status"].tolist() == [RM.CONVERGED, RM.FEW]
    assert 1 < first["iterations"][0] < 12 and first["iterations"][0] < both["iterations"][0] < first["iterations"][0] + 12
    assert both["used"][0].tolist() == [150, 300] and both["sums"][0, 0].tobytes() == first["sums"][0, 0].tobytes()
    assert both["iterations"][1] == 1 and both["used"][1].tolist() == [0, 0] and both["pose"][1].tobytes() == pose_of(R[1], t[1]).tobytes()
    assert both[1].tobytes() == first[1].tobytes()


# ---- the order of the sums ------------------------------------------------------------------------------------------------------------------
def test_the_sums_follow_the_tree_and_depend_on_the_order():
    x = np.array([2.0 ** 53, 1.0, 1.0, -2.0 ** 53] + [0.0] * 126)
    tree = lambda v: float(AM.reduce_tiles(AM.tree64(RM.group_lanes(np.asarray(v, D)[None])))[0])
    assert tree(x) == 1.0 and tree(x[[0, 3, 1, 2] + list(range(4, 130))]) == 2.0
    assert tree(x) == AM.reduce_loop([AM.tree64_loop(list(g)) for g in RM.group_lanes(x)])
    assert RM.group_lanes(np.zeros((28, 0))).shape == (28, 1, 64) and RM.group_lanes(np.zeros(65)).shape == (2, 64)
    far = np.zeros(64 * 65)
    far[[0, 64 * 64]] = 2.0 ** 53, 1.0                        # the second round's first group ends before the last group sum
    far[[63, 64 * 64 + 1]] = -2.0 ** 53, 1.0
    assert tree(far) == 2.0 and tree(far[::-1]) == 2.0 and tree(np.roll(far, 1)) == 2.0
    tg, pts = prototype()
    pose = pose_of(np.eye(3), (0.01, 0, 0.005))
    a, b = RM.system(tg, pts, pose, 1, 0.4, 0.4), RM.system(tg, pts[::-1], pose, 1, 0.4, 0.4)
    assert a[0] == b[0] == 600 and a[1].tobytes() != b[1].tobytes() and np.allclose(a[1], b[1], rtol=1e-9, atol=1e-12)


# ---- convergence ----------------------------------------------------------------------------------------------------------------------------
CONVERGENCE_LEVELS = ((4, 20, 0.4), (2, 20, 0.2), (1, 60, 0.1))


@pytest.mark.parametrize("angle,shift", [(0.04, 0.05), (0.2, 0.2)])
def test_convergence_on_the_prototype_scene(angle, shift):
    tg, pts = prototype()
    R, t = perturbed_starts(2, angle, shift)
    res = RM.align(tg, pts, R, t, levels=CONVERGENCE_LEVELS, eps=1e-7)
    for k in range(2):
        r0, t0 = RM.pose_error(R[k], t[k])
        r1, t1 = RM.pose_error(res["pose"][k, :9], res["pose"][k, 9:])
        print(f"{angle} rad / {shift} m, start {k}: {res['iterations'][k]} systems, used {res['used'][k, 1]}, {r1:.3e} rad, {t1:.3e} m, rms {RM.rms(res)[k]:.3e} m")
        assert res["status"][k] == RM.CONVERGED and res["used"][k, 1] == 600
        assert r1 < r0 and t1 < t0
        assert r1 < 2 * MIRROR_ROTATION and t1 < 2 * MIRROR_TRANSLATION and RM.rms(res)[k] < 2 * MIRROR_RMS


def test_choose_takes_the_principal_start_that_reaches_the_truth():
    """the surface without the half-turn symmetry, the source moved by 2 rad and 3 m, the four principal starts: `choose` returns a start
    that reaches the truth, and a start that does not reach it ends more than 1 rad away with too few points or a residual two orders
    above.  On this sample two of the four reach it (600 used, rms 0.145 mm, 4.3e-4 rad) and two end with 440 and 572 points used and an
    rms above 20 mm; the issue's prototype sample had exactly one winner.  Which of two starts half a turn apart still finds its way
    depends on the sample, so the count of winners is printed and only bounded (at least one, not all four)."""
    tg, truth = prototype(asymmetric=True)
    Rm, tm = RM.perturbation(7, 2.0, 3.0)
    src = ((truth.astype(D) - tm) @ Rm).astype(F)            # (Rm, tm) brings it back
    R0, t0 = RM.principal_starts(src, tg.v)
    assert np.allclose(np.linalg.det(R0), 1) and np.allclose(R0 @ R0.transpose(0, 2, 1), np.eye(3), atol=1e-12)
    res = RM.align(tg, src, R0, t0, levels=((4, 15, 0.4), (2, 10, 0.2), (1, 10, 0.1)))
    errors = [RM.pose_error(res["pose"][k, :9], res["pose"][k, 9:], Rm, tm) for k in range(4)]
    good = [k for k in range(4) if errors[k][0] < 2 * MIRROR_ROTATION]
    print("principal starts:", [(AM.STATUS_NAMES[res["status"][k]], int(res["used"][k, 1]), f"{errors[k][0]:.2e} rad", f"{RM.rms(res)[k]:.2e} m") for k in range(4)])
    g = RM.choose(res)
    assert good and len(good) < 4 and g in good and g == MR.choose(AM.as_dict(res))
    moved = RM.apply(res["pose"][g], src)
    assert res["used"][g, 1] == 600 and RM.rms(res)[g] < 2 * MIRROR_RMS and np.abs(moved - truth).max() < 2e-3
    for k in set(range(4)) - set(good):                       # the others end far away: too few points, or a residual two orders above
        assert errors[k][0] > 1 and (res["status"][k] == RM.FEW or RM.rms(res)[k] > 0.01 or res["used"][k, 1] < 600)


def test_choose_by_hand():
    def result(status, used, error):
        n = len(status)
        return dict(status=np.array(status), used=np.array([[0, u] for u in used], np.uint32), error=np.array([[0.0, e] for e in error]),
                    R=np.zeros((n, 3, 3)), t=np.zeros((n, 3)))
    C, R_, FEW, S = MR.CONVERGED, MR.RUNNING, MR.FEW, MR.SINGULAR
    assert MR.choose(result([C, C, C], [10, 12, 11], [1.0, 5.0, 0.1])) == 1                   # the largest used first
    assert MR.choose(result([C, R_, C], [12, 12, 12], [4.0, 1.0, 2.0])) == 1                  # then the smallest rms; running counts
    assert MR.choose(result([C, C, C], [12, 12, 12], [1.0, 1.0, 1.0])) == 0                   # then the smallest index
    assert MR.choose(result([FEW, S, C], [500, 500, 7], [0.0, 0.0, 3.0])) == 2                # FEW and SINGULAR never
    assert MR.choose(result([FEW, S], [5, 50], [0.0, 0.0])) is None and MR.choose(result([C], [0], [0.0])) is None
    assert MR.rms(result([C], [4], [16.0]))[0] == 2.0 and np.isnan(MR.rms(result([C], [0], [0.0]))[0])
    res = np.zeros(3, RM.RESULT_DTYPE)
    res["status"], res["used"][:, 1], res["sums"][:, 1, 27] = [C, FEW, R_], [9, 99, 9], [2.0, 0.0, 1.0]
    assert RM.choose(res) == MR.choose(AM.as_dict(res)) == 2
    assert MR.RESULT == RM.RESULT_DTYPE and MR.RESULT.itemsize == 560 and MR.STATUS == AM.STATUS_NAMES


# ---- the Python checkers, one by one --------------------------------------------------------------------------------------------------------
def test_capacity_start_level_and_parameter_checkers():
    assert MR.capacity_arg(1, 1, 1, 1, 1) == (1, 1, 1, 1, 1) and MR.capacity_arg(5, 6, 7, 1 << 23, 256) == (5, 6, 7, 1 << 23, 256)
    assert MR.capacity_arg(1, 1, 1, 1 << 31, np.int64(1)) == (1, 1, 1, 1 << 31, 1)
    good = [1, 1, 1, 1, 1]
    for k in range(5):
        for bad in (0, (1 << 31) + 1, -1, 1.0, "1", None, True):
            with pytest.raises(ValueError):
                MR.capacity_arg(*(good[:k] + [bad] + good[k + 1:]))
    for n, s in ((1, 257), ((1 << 23) + 1, 256), (1 << 31, 2)):
        with pytest.raises(ValueError):
            MR.capacity_arg(1, 1, 1, n, s)
    p = MR.starts_arg(np.eye(3), (1, 2, 3))
    assert p.shape == (1, 12) and p.dtype == D and p[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 2, 3] and p.flags.c_contiguous
    assert MR.starts_arg(np.zeros((4, 3, 3)), np.zeros((4, 3)), 4).shape == (4, 12)
    for R, t, cap in ((np.eye(3), (1, 2), 9), (np.zeros((2, 3, 3)), np.zeros((3, 3)), 9), (np.zeros((0, 3, 3)), np.zeros((0, 3)), 9),
                      (np.zeros((3, 3, 3)), np.zeros((3, 3)), 2), (np.eye(3) * NAN, (0, 0, 0), 9), (np.eye(3), (0, INF, 0), 9), ("x", (0, 0, 0), 9),
                      (None, None, 9)):
        with pytest.raises(ValueError):
            MR.starts_arg(R, t, cap)
    d = float(F(0.4))
    assert MR.levels_arg(None, 0.4) == MR.default_levels(0.4) == ((4, 15, d), (2, 15, d / 2), (1, 20, d / 4))
    assert [tuple(l) for l in RM.levels_of(None, 0.4)] == [tuple(l) for l in MR.levels_arg(None, 0.4)]
    assert MR.levels_arg([(3, 256, 0.1)], 0.4) == ((3, 256, float(F(0.1))),) and MR.levels_arg(((1, 1, 0.4),) * 4, 0.4)[3] == (1, 1, d)
    for lv in ((), ((1, 1, 0.1),) * 5, ((0, 1, 0.1),), ((1, 0, 0.1),), ((1, 257, 0.1),), ((1, 200, 0.1), (1, 57, 0.1)), ((1, 1, 0.0),), ((1, 1, -0.1),),
               ((1, 1, NAN),), ((1, 1, INF),), ((1, 1, float(up(0.4))),), ((1, 1),), ((1.0, 1, 0.1),), ((1, True, 0.1),), ((1, 1, "0.1"),), 3, ((1 << 31, 1, 0.1),)):
        with pytest.raises(ValueError):
            MR.levels_arg(lv, 0.4)
    with pytest.raises(ValueError):
        MR.levels_arg(None, NAN)
    for lv in ((), ((1, 1, 0.1),) * 5, ((0, 1, 0.1),), ((1, 0, 0.1),), ((1, 257, 0.1),), ((1, 1, 0.0),), ((1, 1, NAN),), ((1, 1, float(up(0.4))),)):
        with pytest.raises(ValueError):
            RM.levels_of(lv, 0.4)
    assert MR.params_arg(0.1, 0, 1e-7, 6) == (float(F(0.1)), 0.0, 1e-7, 6)
    for bad in ((0, 0, 1e-7, 6), (-1, 0, 1e-7, 6), (NAN, 0, 1e-7, 6), (INF, 0, 1e-7, 6), ("x", 0, 1e-7, 6), (0.1, -1e-9, 1e-7, 6), (0.1, NAN, 1e-7, 6),
                (0.1, INF, 1e-7, 6), (0.1, 0, 0, 6), (0.1, 0, -1, 6), (0.1, 0, NAN, 6), (0.1, 0, 1e-7, 5), (0.1, 0, 1e-7, 6.0), (0.1, 0, 1e-7, 1 << 32),
                (0.1, 0, 1e-7, True), (0.1, True, 1e-7, 6)):
        with pytest.raises(ValueError):
            MR.params_arg(*bad)


def test_checks_come_before_the_library():
    for caps in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 257), (1, 1, 1, 1 << 31, 2)):
        with pytest.raises(ValueError):
            MR.Registration(None, *caps)

    class Ctx:
        device = 0
    r = MR.Registration.__new__(MR.Registration)
    r.ctx, r.max_vertices, r.max_triangles, r.max_pairs, r.max_points, r.max_starts, r.planned, r.needed_pairs = Ctx(), 10, 10, 10, 10, 2, None, None
    for dm in (0, NAN, -1.0, "x"):
        with pytest.raises(ValueError):
            r.target(None, None, dm)
    with pytest.raises(ValueError):
        r.target(None, None, 1.0, cell=1.0)                          # below 1.0625
    with pytest.raises(ValueError):
        r.target(np.zeros((3, 3), F), np.zeros((1, 3), np.int32), 0.1)
    with pytest.raises(ValueError, match="no target"):
        r.align(None, np.eye(3), np.zeros(3))
    r.planned = dict(d_max=float(F(0.4)))
    host = torch.zeros((5, 3), dtype=torch.float32)
    calls = [lambda: r.align(host, np.eye(3), np.zeros(3)), lambda: r.align(None, np.eye(3), np.zeros(3)),
             lambda: r.align_records(torch.zeros((4, 32), dtype=torch.uint8), np.eye(3), np.zeros(3)),
             lambda: r.align(host, np.zeros((3, 3, 3)), np.zeros((3, 3))),                   # more starts than the handle holds
             lambda: r.align(host, np.full((3, 3), INF), np.zeros(3)), lambda: r.align(host, np.eye(3), np.zeros(3), levels=((1, 1, 0.5),)),
             lambda: r.align(host, np.eye(3), np.zeros(3), huber=0), lambda: r.align(host, np.eye(3), np.zeros(3), damping=-1),
             lambda: r.align(host, np.eye(3), np.zeros(3), eps=0), lambda: r.align(host, np.eye(3), np.zeros(3), min_points=5),
             lambda: r.align_into(host, np.eye(3), np.zeros(3), None, None, 0.0, 1e-7, 6, None),
             lambda: r.apply(host, np.eye(3), np.zeros(3)), lambda: r.apply(host, np.full((3, 3), NAN), np.zeros(3)),
             lambda: MR.principal_starts(host, host), lambda: MR.register_points(None, host, host, None, 0.1),
             lambda: MR.register_mesh(None, host, None, host, None, 0.1)]
    r._h = None
    for f in calls:
        with pytest.raises(ValueError):
            f()
    for bad in ("nothing", 3, (1, 2, 3)):
        with pytest.raises(ValueError):
            MR._starts(bad, None, None)
    assert [len(x) for x in MR._starts(None, None, None)] == [1, 1] and MR._starts("identity", None, None)[0][0].tolist() == np.eye(3).tolist()
    lines = MR.pose_lines(dict(R=np.eye(3), t=np.array([0.0, 3.0, 4.0]), start=2, status="converged", iterations=9, used=600, rms=0.00014))
    assert len(lines) == 4 and "start 2 converged after 9 systems, 600 points used" in lines[0] and "translation 5.000000 m" in lines[0]
    assert MR.pose_lines(dict(R=None))[0] == "registration: no start ended converged or running"


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_meshreg.c"
    src.write_text('#include "rgbid_meshreg.h"\n'
                   "int use(rgbid_meshreg* h, rgbid_ctx* ctx, const float* v, const uint32_t* tris, const float* p, const rgbid_cloud_point* rec,\n"
                   "        rgbid_meshreg_result* res, float* out) {\n"
                   "  long long grid[6]; unsigned long long stats[4]; float ms[4]; double pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};\n"
                   "  rgbid_meshreg_level lv[RGBID_MESHREG_MAX_LEVELS] = {{4, 15, 0.4f}, {1, RGBID_MESHREG_MAX_ITERATIONS - 15, 0.1f}};\n"
                   "  return rgbid_meshreg_create(&h, ctx, RGBID_MESHDIST_MAX_VERTICES, RGBID_MESHDIST_MAX_TRIANGLES, RGBID_MESHDIST_MAX_PAIRS,\n"
                   "                              RGBID_MESHREG_MAX_QUERIES / RGBID_MESHREG_MAX_STARTS, RGBID_MESHREG_MAX_STARTS)\n"
                   "       + rgbid_meshreg_target(h, 10, v, 5, tris, 0.4f, 0.f, grid, stats)\n"
                   "       + rgbid_meshreg_align(h, 7, p, 1, pose, 0.4f, 0.0, 1e-7, 6, 2, lv, res)\n"
                   "       + rgbid_meshreg_align_records(h, 7, rec, 1, pose, 0.4f, 0.0, 1e-7, 6, 2, lv, res)\n"
                   "       + rgbid_meshreg_apply(h, 7, p, p, pose, out, out) + rgbid_meshreg_set_query_sort(h, 0) + rgbid_meshreg_timing(h, 1, ms)\n"
                   "       + rgbid_meshreg_destroy(h) + (res[0].status == RGBID_MESHREG_RUNNING) + (res[0].status == RGBID_MESHREG_CONVERGED)\n"
                   "       + (res[0].status == RGBID_MESHREG_FEW) + (res[0].status == RGBID_MESHREG_SINGULAR) + (sizeof(rgbid_meshreg_result) == 560)\n"
                   "       + (sizeof res[0].sums == 2 * RGBID_MESHREG_TERMS * sizeof(double)) + (sizeof(rgbid_meshreg_level) == 12); }\n"
                   "typedef char result_is_560_bytes[sizeof(rgbid_meshreg_result) == 560 ? 1 : -1];\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_meshreg.h")).read()
    const = lambda name: re.search(r"#define RGBID_MESHREG_%s\s+(\w+)" % name, txt).group(1)
    assert int(const("MAX_STARTS")) == MR.MAX_STARTS == RM.MAX_STARTS and const("MAX_QUERIES") == "2147483648ull" and MR.MAX_QUERIES == 1 << 31
    assert int(const("MAX_LEVELS")) == MR.MAX_LEVELS == RM.MAX_LEVELS and int(const("MAX_ITERATIONS")) == MR.MAX_ITERATIONS == RM.MAX_ITERATIONS
    assert int(const("TERMS")) == MR.TERMS == RM.TERMS and int(const("NAN_BITS")[:-3], 16) == int(AM.NAN_BITS)
    for k, name in enumerate(("RUNNING", "CONVERGED", "FEW", "SINGULAR")):
        assert int(re.search(r"RGBID_MESHREG_%s = (\d)" % name, txt).group(1)) == k == getattr(MR, name) == getattr(RM, name) and MR.STATUS[k] == name.lower()
    assert ctypes.sizeof(MR.Level) == 12
    # the result record is laid out as section 21's
    tsdf = open(os.path.join(ROOT, "include", "rgbid_tsdf_align.h")).read()
    fields = lambda t, name: re.findall(r"^\s+(\w+) (\w+(?:\[\w+\])*);", re.search(r"typedef struct %s \{(.*?)\}" % name, t, re.S).group(1), re.M)
    assert [(a, b.replace("RGBID_MESHREG_", "")) for a, b in fields(txt, "rgbid_meshreg_result")] == \
           [(a, b.replace("RGBID_TSDF_ALIGN_", "")) for a, b in fields(tsdf, "rgbid_tsdf_align_result")]


def test_library_exports_meshreg_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_meshreg.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_meshreg_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(MR.MESHREG_EXPORTS) == set(MR.SIGNATURES) and len(declared) == 8, set(declared) ^ set(MR.MESHREG_EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    for name, types in MR.SIGNATURES.items():
        getattr(L, name).argtypes = list(types)
    h = c.c_void_p()
    assert L.rgbid_meshreg_create(c.byref(h), None, 10, 10, 10, 10, 2) == -1 and not h.value and L.rgbid_meshreg_create(None, None, 10, 10, 10, 10, 2) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    big = (1 << 31) + 1
    for caps in ((0, 10, 10, 10, 2), (10, 0, 10, 10, 2), (10, 10, 0, 10, 2), (10, 10, 10, 0, 2), (10, 10, 10, 10, 0), (big, 10, 10, 10, 2), (10, big, 10, 10, 2),
                 (10, 10, big, 10, 2), (10, 10, 10, big, 1), (10, 10, 10, 10, 257), (10, 10, 10, (1 << 23) + 1, 256), (10, 10, 10, 1 << 31, 2),
                 (10, 10, 10, 1 << 62, 4)):
        assert L.rgbid_meshreg_create(c.byref(h), fake, *caps) == -1 and not h.value, caps
    pose = (c.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    lv = (MR.Level * 1)(MR.Level(1, 1, 0.1))
    assert L.rgbid_meshreg_target(None, 0, None, 0, None, 0.1, 0.0, None, None) == -1
    assert L.rgbid_meshreg_align(None, 0, None, 1, pose, 0.1, 0.0, 1e-7, 6, 1, lv, None) == -1
    assert L.rgbid_meshreg_align_records(None, 0, None, 1, pose, 0.1, 0.0, 1e-7, 6, 1, lv, None) == -1
    assert L.rgbid_meshreg_apply(None, 0, None, None, pose, None, None) == -1
    assert L.rgbid_meshreg_set_query_sort(None, 1) == -1
    assert L.rgbid_meshreg_timing(None, 0, None) == -1 and L.rgbid_meshreg_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((mesh_opt + ["--mesh-reference-register"], "--mesh-reference-register needs --mesh-reference"),
                      (["--mesh-reference", "x.ply", "--mesh-reference-register"], "need --mesh"),
                      (mesh_opt + ["--mesh-reference", str(tmp_path / "absent.ply"), "--mesh-reference-register"], "--mesh-reference: cannot read")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()
    tool = os.path.join(ROOT, "tools", "mesh_compare.py")
    a = str(tmp_path / "a.ply")
    for bad, word in (([a, a, "--max-distance", "1", "--starts", "principal"], "--starts / --out-aligned need --register"),
                      ([a, a, "--max-distance", "1", "--register", "--starts", "random"], "invalid choice"),
                      ([a, a, "--max-distance", "0", "--register"], "d_max must be finite and > 0"),
                      ([a, a, "--max-distance", "1", "--register", "--starts", "principal", "--out-aligned", str(tmp_path / "c.ply")], "cannot read")):
        r = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "c.ply").exists()
