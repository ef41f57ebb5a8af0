"""GPU tests of the registration stage (include/rgbid_meshreg.h, csrc/kernels_meshreg.hip, rgbid.meshreg): every byte of the result records
(poses, status, systems built, used counts, both sets of sums) and of apply's output against tests/meshreg_mirror.py, with canaries behind
every buffer: the prototype scene from 1, 3 and 17 starts; point counts either side of the minimum, of the wave and of one, two and three
rounds of the upper tree; strides; three levels with the Huber threshold below the reach, damping and a coarse eps; every threshold case
of tests/test_cpu_meshreg.py; five starts that end in every status in one call; records; the query sort on and off; targets of every size
on one handle; every refusal with the handle used afterwards; the stage timer; and the composites: register_mesh and the command lines."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import _lib
from rgbid import meshdist as MD
from rgbid import meshreg as MR
from rgbid import tsdf as TS
from tests import align_mirror as AM
from tests import meshdist_mirror as DM
from tests import meshreg_mirror as RM
from tests.test_cpu_meshreg import IDENTITY, PLANE_T, PLANE_V, perturbed_starts, plane_target, pose_of, prototype, small_scene, up

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D, U32 = np.float32, np.float64, np.uint32
NAN, INF = float("nan"), float("inf")
CAP_V, CAP_T, CAP_P, CAP_N, CAP_S = 1000, 2000, 40000, 4200, 17
PAD = 64                                                    # bytes behind the records that must keep their canary
CANARY = 0xA5


@pytest.fixture(scope="module")
def reg(ctx):
    """one handle for the whole file: every test reuses it for a target of another size"""
    h = MR.Registration(ctx, CAP_V, CAP_T, CAP_P, CAP_N, CAP_S)
    yield h
    h.close()


def dev(a):
    a = np.ascontiguousarray(a)
    a = a.astype(U32) if a.dtype == np.int64 else a
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def records_of(points):
    """rgbid_cloud_point records with the positions of float32 [n, 3] and other bytes elsewhere"""
    rec = np.full((len(points), 8), 0x5A5A5A5A, U32)
    rec[:, :3] = np.ascontiguousarray(points, F).view(U32)
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 32)).cuda()


def set_target(reg, tg, cell=None):
    got = reg.target(dev(tg.v), dev(tg.t), float(tg.d_max), cell)
    exp = DM.plan(tg.v, tg.t, tg.d_max, cell)
    assert got["grid"] == exp["grid"].tolist() and {k: got[k] for k in MD.STATS} == {k: exp[k] for k in MD.STATS}
    return got


def run(reg, pts, R, t, records=False, levels=None, huber=None, damping=0.0, eps=1e-7, min_points=6):
    """one align into a buffer with PAD canary bytes behind the V records -> the records as numpy"""
    V = len(np.asarray(R, D).reshape(-1, 9))
    buf = torch.full((V * 560 + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    p = records_of(pts) if records else dev(np.ascontiguousarray(pts, F).reshape(-1, 3))
    reg.ctx.wait_torch_stream()
    reg.align_into(p, R, t, levels, huber, damping, eps, min_points, buf[:V * 560], records)
    reg.ctx.sync()
    assert (buf[V * 560:] == CANARY).all()
    return buf[:V * 560].cpu().numpy().view(RM.RESULT_DTYPE)


def differences(got, exp):
    """the fields and starts at which two sets of records differ"""
    return [(k, v) for v in range(len(exp)) for k in exp.dtype.names if got[k][v].tobytes() != exp[k][v].tobytes()]


def assert_aligned(reg, tg, pts, R, t, exp=None, **kw):
    exp = RM.align(tg, pts, R, t, **kw) if exp is None else exp
    got = run(reg, pts, R, t, **kw)
    assert got.tobytes() == exp.tobytes(), (differences(got, exp), got["status"], exp["status"], got["iterations"], exp["iterations"], got["used"], exp["used"])
    return exp


# ---- the prototype scene ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prototype_mirror():
    """17 perturbed starts over two levels, once for the tests that share it"""
    tg, pts = prototype()
    R, t = perturbed_starts(17, 0.04, 0.05)
    levels = ((4, 2, 0.4), (1, 1, 0.2))
    return R, t, levels, RM.align(tg, pts, R, t, levels=levels)


@pytest.mark.parametrize("V", [1, 3, 17])
def test_prototype_scene(reg, V):
    tg, pts = prototype()
    R, t, levels, exp = prototype_mirror()
    set_target(reg, tg)
    assert_aligned(reg, tg, pts, R[:V], t[:V], exp[:V], levels=levels)
    assert (exp["iterations"] == 3).all() and (exp["used"][:, 1] == 600).all() and (exp["status"] == RM.RUNNING).all()


def test_records_and_the_query_sort(reg):
    tg, pts = prototype()
    R, t, levels, exp = prototype_mirror()
    set_target(reg, tg)
    for sort in (False, True):
        reg.sort_queries(sort)
        assert run(reg, pts, R[:3], t[:3], levels=levels).tobytes() == exp[:3].tobytes()
        assert run(reg, pts, R[:3], t[:3], records=True, levels=levels).tobytes() == exp[:3].tobytes()
    got = reg.align_records(records_of(pts), R[:2], t[:2], levels=levels)                  # the wrapper, as a dict
    want = AM.as_dict(exp[:2])
    assert sorted(got) == sorted(want) and all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want)


@pytest.mark.parametrize("stride", [1, 2, 3, 8])
def test_strides(reg, stride):
    tg, pts = prototype()
    R, t = perturbed_starts(2, 0.04, 0.05)
    set_target(reg, tg)
    exp = assert_aligned(reg, tg, pts[:599], R, t, levels=((stride, 2, 0.4),))
    assert (exp["used"][:, 1] == (599 + stride - 1) // stride).all()


def test_three_levels_huber_damping_and_eps(reg):
    tg, pts = prototype()
    R, t = perturbed_starts(3, 0.1, 0.1)
    set_target(reg, tg)
    exp = assert_aligned(reg, tg, pts, R, t, levels=((4, 6, 0.4), (2, 4, 0.2), (1, 3, 0.1)), huber=0.002, damping=1e-3, eps=1e-4)
    assert (exp["iterations"] > 6).all() and (exp["used"][:, 0] <= 150).all() and (exp["used"][:, 1] > 500).all()


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 5, 6, 63, 64, 65])
def test_point_counts_around_the_minimum_and_the_wave(reg, n):
    tg, _ = small_scene()
    pts = RM.surface_points(65, seed=12).astype(F)[:n]
    R, t = perturbed_starts(2, 0.02, 0.02)
    set_target(reg, tg)
    exp = assert_aligned(reg, tg, pts, R, t, levels=((1, 2, 0.4),))
    assert (exp["status"] == RM.FEW).all() == (n < 6) and (exp["used"][:, 0] == n).all()


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_one_and_two_rounds_of_the_upper_tree(reg, n):
    tg, _ = small_scene()
    pts = RM.surface_points(4097, seed=13).astype(F)[:n]
    R, t = perturbed_starts(2, 0.02, 0.02)
    set_target(reg, tg)
    exp = assert_aligned(reg, tg, pts, R, t, levels=((1, 2, 0.4),))
    assert (exp["used"] == n).all() and (exp["iterations"] == 2).all()


def test_three_rounds_of_the_upper_tree(ctx):
    """262 145 points are 4 097 groups: three rounds.  The target has two triangles, so the brute-force mirror stays cheap"""
    n = 262145
    v = np.array([(-2, -2, 0), (2, -2, 0), (0, 2, 1), (4, 2, -1)], F)                       # a roof: two normals
    tg = RM.Target(v, np.array([(0, 1, 2), (1, 3, 2)]), 0.25)
    r = np.random.default_rng(14)
    a, b = r.uniform(0, 1, n), r.uniform(0, 1, n)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    tri = r.integers(0, 2, n)
    c = v[tg.t[tri]].astype(D)
    pts = (c[:, 0] + a[:, None] * (c[:, 1] - c[:, 0]) + b[:, None] * (c[:, 2] - c[:, 0]) + r.normal(0, 0.02, (n, 3))).astype(F)
    pts[::1001] = (NAN, 0, 0)
    R, t = perturbed_starts(1, 0.01, 0.01, seed=5)
    h = MR.Registration(ctx, 4, 2, 4096, n, 1)
    set_target(h, tg)
    exp = assert_aligned(h, tg, pts, R, t, levels=((1, 1, 0.25), (2, 1, 0.125)), damping=1e-6)
    assert exp["used"][0, 0] > 250000 and exp["iterations"][0] in (1, 2)
    h.close()


# ---- the thresholds of the CPU file -------------------------------------------------------------------------------------------------------------
def test_reach_and_huber_to_the_ulp(reg):
    tg = plane_target()
    set_target(reg, tg)
    one = lambda z: np.array([(0.3, 0.2, z)], F)
    for z, reach, huber, used in ((0.125, 0.125, 0.5, 1), (up(0.125), 0.125, 0.5, 0), (0.125, float(up(0.125, 0)), 0.5, 0), (-0.125, 0.125, 0.5, 1),
                                  (0.125, 0.5, 0.125, 1), (up(0.125), 0.5, 0.125, 1), (0.125, 0.5, float(up(0.125, 0)), 1)):
        exp = assert_aligned(reg, tg, one(z), np.eye(3), np.zeros(3), levels=((1, 1, reach),), huber=huber)
        assert exp["status"][0] == RM.FEW and exp["used"].tolist() == [[used, used]] and (exp["sums"][0, 0, 27] > 0) == bool(used)


def test_degenerate_winners_and_non_finite_points(reg):
    v = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0.5, 0.5, 0.5)], F)
    r = np.random.default_rng(15)
    pts = (np.array([(0.5, 0.4, 0.4)]) + r.normal(0, 0.05, (40, 3))).astype(F)
    for tri in ([(3, 3, 3)], [(0, 1, 2)], [(0, 2, 1)], [(3, 3, 3), (0, 1, 2)]):
        tg = RM.Target(v, np.array(tri), 1.0)
        set_target(reg, tg)
        exp = assert_aligned(reg, tg, pts, np.eye(3), np.zeros(3), levels=((1, 2, 1.0),), huber=0.5)
        assert exp["status"][0] == RM.FEW and exp["used"].tolist() == [[0, 0]] and (tg.query(pts)["triangle"] != RM.NONE).all()
    v = np.array(PLANE_V + [(0, 0, NAN), (1, 1, INF)], F)                                  # triangles that take no part beside two that do
    tg = RM.Target(v, np.array(PLANE_T + [(0, 1, 4), (5, 2, 3)]), 0.5)
    set_target(reg, tg)
    assert_aligned(reg, tg, pts, np.eye(3), np.zeros(3), levels=((1, 1, 0.5),))
    tg, pts = small_scene()
    bad = pts.copy()
    bad[[3, 17, 40]] = [(NAN, 0, 1.8), (0, INF, 1.8), (0, 0, -INF)]
    R, t = perturbed_starts(2, 0.02, 0.02)
    set_target(reg, tg)
    exp = assert_aligned(reg, tg, bad, R, t, levels=((1, 3, 0.4),))
    assert (exp["used"] == 67).all()
    exp = assert_aligned(reg, tg, pts[:8], np.eye(3) * 3e38, np.zeros(3), levels=((1, 1, 0.4),))   # a finite pose, points that overflow float32
    assert exp["status"][0] == RM.FEW and exp["used"][0, 0] == 0


def test_min_points_flat_targets_and_restarts(reg):
    tg, pts = small_scene()
    R, t = perturbed_starts(1, 0.01, 0.01)
    set_target(reg, tg)
    ok = assert_aligned(reg, tg, pts[:6], R, t, levels=((1, 2, 0.4),), min_points=6)
    few = assert_aligned(reg, tg, pts[:6], R, t, levels=((1, 2, 0.4),), min_points=7)
    assert ok["status"][0] != RM.FEW and few["status"][0] == RM.FEW and few["pose"][0].tobytes() == pose_of(R[0], t[0]).tobytes()
    flat = plane_target()
    r = np.random.default_rng(4)
    fp = np.c_[r.uniform(-1, 1, (40, 2)), np.full(40, 0.01)].astype(F)
    set_target(reg, flat)
    exp = assert_aligned(reg, flat, fp, R, [(0.01, -0.02, 0.03)], levels=((1, 3, 0.5),), damping=1e-3)
    assert exp["status"][0] == RM.SINGULAR and exp["iterations"][0] == 1 and exp["pose"][0].tobytes() == pose_of(R[0], (0.01, -0.02, 0.03)).tobytes()
    tg, pts = prototype()
    R = np.concatenate([R, np.eye(3)[None]]); t = np.concatenate([t, [(0, 0, 5.0)]])
    set_target(reg, tg)
    exp = assert_aligned(reg, tg, pts, R, t, levels=((4, 12, 0.4), (2, 12, 0.2)), eps=1e-4)
    assert exp["status"].tolist() == [RM.CONVERGED, RM.FEW] and 2 < exp["iterations"][0] < 24 and exp["iterations"][1] == 1


def test_five_starts_end_in_every_way(reg):
    """two starts that meet eps before a level's end, one without a point in reach, one on a flat patch, one that uses every iteration"""
    tg0, pts = prototype()
    n = len(tg0.v)
    v = np.concatenate([tg0.v, np.array([(-4, -4, 10), (4, -4, 10), (4, 4, 10), (-4, 4, 10)], F)])
    tg = RM.Target(v, np.concatenate([tg0.t, [(n, n + 1, n + 2), (n, n + 2, n + 3)]]), 0.4)
    Rn, tn = perturbed_starts(2, 0.004, 0.004)
    R = np.stack([Rn[0], np.eye(3), Rn[1], np.eye(3), np.eye(3)])
    t = np.stack([tn[0], (0, 0, 5.0), tn[1], (0, 0, 8.3), (1.5, 0.3, 0.15)])
    set_target(reg, tg)
    exp = assert_aligned(reg, tg, pts, R, t, levels=((4, 4, 0.4), (2, 6, 0.2)), eps=1e-4)
    assert exp["status"].tolist() == [RM.CONVERGED, RM.FEW, RM.CONVERGED, RM.SINGULAR, RM.RUNNING], exp["status"]
    assert exp["iterations"][[1, 3, 4]].tolist() == [1, 1, 10] and (exp["iterations"][[0, 2]] < 9).all() and (exp["iterations"][[0, 2]] > 2).all()
    assert exp["pose"][1].tobytes() == pose_of(R[1], t[1]).tobytes() and exp["pose"][3].tobytes() == pose_of(R[3], t[3]).tobytes()


# ---- one handle, many calls ---------------------------------------------------------------------------------------------------------------------
def test_targets_of_every_size_and_repeated_calls(reg):
    big, pts = prototype()
    small, spts = small_scene()
    R, t, levels, exp = prototype_mirror()
    sexp = RM.align(small, spts, R[:2], t[:2], levels=((1, 2, 0.4),))
    set_target(reg, big)
    assert run(reg, pts, R[:2], t[:2], levels=levels).tobytes() == exp[:2].tobytes()
    set_target(reg, small)                                                                 # a smaller target after a larger one
    assert run(reg, spts, R[:2], t[:2], levels=((1, 2, 0.4),)).tobytes() == sexp.tobytes()
    assert run(reg, spts, R[:2], t[:2], levels=((1, 2, 0.4),)).tobytes() == sexp.tobytes()   # twice on one target
    set_target(reg, big, cell=0.6)                                                         # another grid, the same answers
    assert run(reg, pts, R[:3], t[:3], levels=levels).tobytes() == exp[:3].tobytes()
    empty = RM.Target(np.zeros((3, 3), F), np.zeros((0, 3), np.int64), 0.4)                # no triangle: nobody has a winner
    got = reg.target(dev(empty.v), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 0.4)
    assert got["pairs"] == 0
    res = assert_aligned(reg, empty, pts, R[:2], t[:2], levels=levels)
    assert (res["status"] == RM.FEW).all()
    # two calls enqueued back to back, read after one wait
    set_target(reg, big)
    bufs = [torch.full((2 * 560,), CANARY, dtype=torch.uint8, device="cuda") for _ in range(2)]
    p = dev(pts)
    reg.ctx.wait_torch_stream()
    reg.align_into(p, R[:2], t[:2], levels, None, 0.0, 1e-7, 6, bufs[0])
    reg.align_into(p, R[2:4], t[2:4], levels, None, 0.0, 1e-7, 6, bufs[1])
    reg.ctx.sync()
    assert bufs[0].cpu().numpy().tobytes() == exp[:2].tobytes() and bufs[1].cpu().numpy().tobytes() == exp[2:4].tobytes()


def test_apply_against_the_mirror(reg):
    r = np.random.default_rng(16)
    for n in (0, 1, 255, 256, 70001):
        pts = r.normal(0, 2, (n, 3)).astype(F)
        nrm = r.normal(0, 1, (n, 3)).astype(F)
        if n > 1:
            pts[1] = (NAN, 1, INF)
        R, t = RM.perturbation(n, 1.0, 2.0)
        pose = pose_of(R, t)
        ep, en = RM.apply(pose, pts, nrm)
        out = torch.full((n + 3, 3), -7.0, dtype=torch.float32, device="cuda")
        nout = torch.full((n + 3, 3), -9.0, dtype=torch.float32, device="cuda")
        dp, dn = dev(pts), dev(nrm)
        ptr = lambda x: C.c_void_p(x.data_ptr() if x.numel() else 0)
        reg.ctx.wait_torch_stream()
        pose_c = (C.c_double * 12)(*pose)
        _lib.check(reg.L.rgbid_meshreg_apply(reg._h, C.c_ulonglong(n), ptr(dp), ptr(dn), pose_c, ptr(out), ptr(nout) if n else None))   # no normals in, none out
        reg.ctx.sync()
        assert out[:n].cpu().numpy().tobytes() == ep.tobytes() and nout[:n].cpu().numpy().tobytes() == en.tobytes()
        assert (out[n:] == -7.0).all() and (nout[n:] == -9.0).all()
        if n:
            got = reg.apply(dp, R, t)
            assert got.cpu().numpy().tobytes() == ep.tobytes()
            gp, gn = reg.apply(dp, R, t, dn)
            assert gp.cpu().numpy().tobytes() == ep.tobytes() and gn.cpu().numpy().tobytes() == en.tobytes()
            _lib.check(reg.L.rgbid_meshreg_apply(reg._h, C.c_ulonglong(n), ptr(dp), ptr(dn), pose_c, ptr(dp), ptr(dn)))      # in place
            reg.ctx.sync()
            assert dp.cpu().numpy().tobytes() == ep.tobytes() and dn.cpu().numpy().tobytes() == en.tobytes()


def test_stage_timer(ctx):
    tg, pts = prototype()
    R, t, levels, exp = prototype_mirror()
    h = MR.Registration(ctx, CAP_V, CAP_T, CAP_P, 600, 3)
    set_target(h, tg)
    assert h.timing(True) == dict.fromkeys(MR.STAGES, 0.0)
    assert run(h, pts, R[:3], t[:3], levels=levels).tobytes() == exp[:3].tobytes()
    ms = h.timing(False)
    assert all(ms[k] > 0 for k in MR.STAGES), ms
    assert run(h, pts, R[:3], t[:3], levels=levels).tobytes() == exp[:3].tobytes()
    assert h.timing(False) == dict.fromkeys(MR.STAGES, 0.0)
    h.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_reuse(reg):
    tg, pts = prototype()
    R, t, levels, exp = prototype_mirror()
    set_target(reg, tg)
    L, h = reg.L, reg._h
    p, rec = dev(pts), records_of(pts)
    n = len(pts)
    buf = torch.full((2 * 560 + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    poses = np.ascontiguousarray(np.concatenate([R[:2].reshape(2, 9), t[:2]], 1))
    lv = lambda *rows: (MR.Level * len(rows))(*[MR.Level(*r) for r in rows])
    good = dict(f=L.rgbid_meshreg_align, n=n, p=p.data_ptr(), V=2, poses=poses, huber=0.4, damping=0.0, eps=1e-7, min_points=6, levels=lv((4, 2, 0.4), (1, 1, 0.2)),
                n_levels=2, res=buf.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        ps = a["poses"]
        return a["f"](h, C.c_ulonglong(a["n"]), C.c_void_p(a["p"]), a["V"], None if ps is None else ps.ctypes.data_as(C.c_void_p), C.c_float(a["huber"]),
                      C.c_double(a["damping"]), C.c_double(a["eps"]), a["min_points"], a["n_levels"], a["levels"], C.c_void_p(a["res"]))

    def poisoned(k, x):
        q = poses.copy()
        q[1, k] = x
        return q
    d_up = float(up(0.4))
    bad = [dict(n=CAP_N + 1), dict(p=0), dict(p=p.data_ptr() + 2), dict(f=L.rgbid_meshreg_align_records, p=rec.data_ptr(), n=CAP_N + 1),
           dict(f=L.rgbid_meshreg_align_records, p=0), dict(f=L.rgbid_meshreg_align_records, p=rec.data_ptr() + 4), dict(V=0), dict(V=-1), dict(V=CAP_S + 1),
           dict(poses=None), dict(poses=poisoned(0, NAN)), dict(poses=poisoned(11, INF)), dict(poses=poisoned(5, -INF)),
           dict(huber=0.0), dict(huber=-1.0), dict(huber=NAN), dict(huber=INF), dict(damping=-1e-9), dict(damping=NAN), dict(damping=INF),
           dict(eps=0.0), dict(eps=-1.0), dict(eps=NAN), dict(eps=INF), dict(min_points=5), dict(min_points=0),
           dict(n_levels=0), dict(n_levels=5), dict(n_levels=-1), dict(levels=None),
           dict(levels=lv((0, 2, 0.4), (1, 1, 0.2))), dict(levels=lv((-1, 2, 0.4), (1, 1, 0.2))), dict(levels=lv((4, 0, 0.4), (1, 1, 0.2))),
           dict(levels=lv((4, 2, 0.4), (1, -1, 0.2))), dict(levels=lv((4, 200, 0.4), (1, 57, 0.2))), dict(levels=lv((4, 257, 0.4)), n_levels=1),
           dict(levels=lv((4, 2, 0.0), (1, 1, 0.2))), dict(levels=lv((4, 2, -0.1), (1, 1, 0.2))), dict(levels=lv((4, 2, 0.4), (1, 1, NAN))),
           dict(levels=lv((4, 2, INF), (1, 1, 0.2))), dict(levels=lv((4, 2, d_up), (1, 1, 0.2))),
           dict(res=0), dict(res=buf.data_ptr() + 4)]
    reg.ctx.wait_torch_stream()
    for kw in bad:
        assert call(**kw) == -1, kw
    reg.ctx.sync()
    assert (buf == CANARY).all()                                                           # nothing written ...
    assert call() == 0                                                                     # ... and the handle usable
    reg.ctx.sync()
    assert buf[:2 * 560].cpu().numpy().tobytes() == exp[:2].tobytes() and (buf[2 * 560:] == CANARY).all()
    assert call(levels=lv((4, 200, 0.4), (1, 56, 0.2))) == 0 and call(min_points=6, V=1) == 0   # the bounds themselves pass
    reg.ctx.sync()
    # apply
    out = torch.full((n + 2, 3), -7.0, dtype=torch.float32, device="cuda")
    pose = (C.c_double * 12)(*IDENTITY)
    nanpose = (C.c_double * 12)(*([NAN] + list(IDENTITY[1:])))
    ap = lambda cnt, a, b, ps, c, d: L.rgbid_meshreg_apply(h, C.c_ulonglong(cnt), C.c_void_p(a), C.c_void_p(b), ps, C.c_void_p(c), C.c_void_p(d))
    pp, oo = p.data_ptr(), out.data_ptr()
    for args in ((n, 0, 0, pose, oo, 0), (n, pp, 0, pose, 0, 0), (n, pp + 2, 0, pose, oo, 0), (n, pp, 0, pose, oo + 2, 0), (n, pp, pp, pose, oo, 0),
                 (n, pp, 0, pose, oo, oo), (n, pp, pp + 1, pose, oo, oo), (n, pp, 0, None, oo, 0), (n, pp, 0, nanpose, oo, 0), ((1 << 31) + 1, pp, 0, pose, oo, 0)):
        assert ap(*args) == -1, args
    reg.ctx.sync()
    assert (out == -7.0).all()
    assert ap(n, pp, 0, pose, oo, 0) == 0 and ap(0, 0, 0, pose, 0, 0) == 0
    reg.ctx.sync()
    assert out[:n].cpu().numpy().tobytes() == pts.tobytes() and (out[n:] == -7.0).all()
    # the wrapper refuses what the library would, before it
    for f in (lambda: reg.align(p, R[:CAP_S + 1].repeat(2, 0), t[:CAP_S + 1].repeat(2, 0)), lambda: reg.align(p, R[:1], t[:1], levels=((1, 1, d_up),)),
              lambda: reg.align(torch.zeros((CAP_N + 1, 3), device="cuda"), R[:1], t[:1]), lambda: reg.align(p.cpu(), R[:1], t[:1]),
              lambda: reg.align_into(p, R[:1], t[:1], None, None, 0.0, 1e-7, 6, buf[4:564])):
        with pytest.raises(ValueError):
            f()


def test_target_refusals_keep_or_lose_the_former_target(ctx):
    tg, pts = small_scene()
    R, t = perturbed_starts(2, 0.02, 0.02)
    levels = ((1, 2, 0.4),)
    exp = RM.align(tg, pts, R, t, levels=levels)
    h = MR.Registration(ctx, 100, 200, 3000, 100, 2)
    buf = torch.full((2 * 560,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="no target"):
        h.align(dev(pts), R, t)
    poses = np.ascontiguousarray(np.concatenate([R.reshape(2, 9), t], 1))
    p = dev(pts)
    raw = lambda: h.L.rgbid_meshreg_align(h._h, C.c_ulonglong(len(pts)), C.c_void_p(p.data_ptr()), 2, poses.ctypes.data_as(C.c_void_p), C.c_float(0.4),
                                          C.c_double(0.0), C.c_double(1e-7), 6, 1, (MR.Level * 1)(MR.Level(1, 2, 0.4)), C.c_void_p(buf.data_ptr()))
    assert raw() == -1                                                                     # no target yet
    set_target(h, tg)
    v, tr = dev(tg.v), dev(tg.t)
    n_v, n_t = v.shape[0], tr.shape[0]
    grid, stats = (C.c_longlong * 6)(*([77] * 6)), (C.c_ulonglong * 4)(*([77] * 4))
    target = lambda nv, pv, nt, pt, d, c: h.L.rgbid_meshreg_target(h._h, C.c_ulonglong(nv), C.c_void_p(pv), C.c_ulonglong(nt), C.c_void_p(pt), C.c_float(d),
                                                                    C.c_float(c), grid, stats)
    pv, pt = v.data_ptr(), tr.data_ptr()
    for args in ((101, pv, n_t, pt, 0.4, 0), (n_v, pv, 201, pt, 0.4, 0), (n_v, 0, n_t, pt, 0.4, 0), (n_v, pv, n_t, 0, 0.4, 0), (n_v, pv + 2, n_t, pt, 0.4, 0),
                 (n_v, pv, n_t, pt + 1, 0.4, 0), (0, 0, n_t, pt, 0.4, 0), (n_v, pv, n_t, pt, 0.0, 0), (n_v, pv, n_t, pt, NAN, 0), (n_v, pv, n_t, pt, 2.0 ** 61, 0),
                 (n_v, pv, n_t, pt, 0.4, 0.4), (n_v, pv, n_t, pt, 0.4, -1.0), (n_v, pv, n_t, pt, 0.4, NAN)):
        assert target(*args) == -1, args
        assert list(grid) == [77] * 6 and list(stats) == [77] * 4                          # nothing written ...
        assert run(h, pts, R, t, levels=levels).tobytes() == exp.tobytes()                 # ... and the former target kept
    # refused after the first launches: the former target is gone, the handle usable
    tb = tg.t.copy()
    tb[n_t // 2, 1] = n_v
    with pytest.raises(_lib.RgbidError):
        h.target(v, dev(tb), 0.4)
    assert raw() == -1 and h.planned is None
    set_target(h, tg)
    assert run(h, pts, R, t, levels=levels).tobytes() == exp.tobytes()
    fine, _ = prototype()                                                                  # more pairs than the handle holds
    hb = MR.Registration(ctx, 1000, 2000, 1000, 100, 2)
    with pytest.raises(_lib.RgbidError, match="needs"):
        hb.target(dev(fine.v), dev(fine.t), 0.4)
    assert hb.needed_pairs == DM.plan(fine.v, fine.t, 0.4)["pairs"] > 1000
    set_target(hb, tg)
    assert run(hb, pts, R, t, levels=levels).tobytes() == exp.tobytes()
    hb.close()
    h.close()


# ---- composites ---------------------------------------------------------------------------------------------------------------------------------
def moved_copy():
    """the prototype's mesh and a copy of it moved rigidly away by a small motion -> (v, t, moved vertices, the pose that brings them back)"""
    tg, _ = prototype()
    Rm, tm = RM.perturbation(21, 0.1, 0.1)
    return tg.v, tg.t, ((tg.v.astype(D) - tm) @ Rm).astype(F), Rm, tm


def test_register_mesh_and_principal_starts(ctx):
    v, t, va, Rm, tm = moved_copy()
    tg, _ = prototype()
    levels = ((4, 8, 0.4), (2, 6, 0.2), (1, 6, 0.1))
    exp = RM.align(tg, va, np.eye(3)[None], np.zeros((1, 3)), levels=levels)
    got = MR.register_mesh(ctx, dev(va), dev(t), dev(v), dev(t), 0.4, levels=levels)
    assert got["start"] == 0 and got["status"] == RM.STATUS_NAMES[exp["status"][0]] and got["iterations"] == exp["iterations"][0]
    assert np.concatenate([got["R"].reshape(9), got["t"]]).tobytes() == exp["pose"][0].tobytes() and got["used"] == exp["used"][0, 1]
    moved = RM.apply(exp["pose"][0], va)
    assert got["points"].cpu().numpy().tobytes() == moved.tobytes()
    # the deviation after is that of the mirror's pose, and every named vertex is within the mirror's figure
    summary = lambda a, ta, b: MD.summary(torch.from_numpy(DM.query(a, ta, b, 0.4)["distance"]))
    for word, pts in (("before", va), ("after", moved)):
        a_to_b, b_to_a = summary(v, t, pts), summary(pts, t, v)
        for one, want in ((got[word]["a_to_b"], a_to_b), (got[word]["b_to_a"], b_to_a)):
            assert one["queries"] == want["queries"] and one["matched"] == want["matched"] > 0
            assert all(one[k] == pytest.approx(want[k], rel=1e-12) for k in ("mean", "rms")) and all(one[k] == want[k] for k in ("median", "p90", "max"))
    r1, t1 = RM.pose_error(got["R"], got["t"], Rm, tm)
    away = np.abs(moved - v).max()
    print(f"register_mesh: {got['status']} after {got['iterations']} systems, {r1:.3e} rad, {t1:.3e} m from the motion, vertices within {away:.3e} m; "
          f"rms before {got['before']['a_to_b']['rms']:.6f} m, after {got['after']['a_to_b']['rms']:.6f} m")
    assert got["after"]["a_to_b"]["rms"] < got["before"]["a_to_b"]["rms"] / 20 and got["after"]["a_to_b"]["matched"] == len(v)
    assert np.abs(got["points"].cpu().numpy() - v).max() == away < 1e-6      # the copy is the mesh itself: what is left is four float32 ulps at 2 m
    # principal starts against the mirror's: the same four poses up to rounding, and a one-shot over them
    Rp, tp = MR.principal_starts(dev(va), dev(v))
    Re, te = RM.principal_starts(va, v)
    match = [int(np.argmin([np.abs(Rp[i] - Re[j]).max() for j in range(4)])) for i in range(4)]      # an eigenvector's sign is the solver's: the same four, in any order
    assert sorted(match) == [0, 1, 2, 3] and np.abs(Rp - Re[match]).max() < 1e-9 and np.abs(tp - te[match]).max() < 1e-9 and np.allclose(np.linalg.det(Rp), 1)
    one = MR.register_points(ctx, dev(va), dev(v), dev(t), 0.4, starts="principal", levels=levels)
    assert one["R"] is not None and MR.choose(one["result"]) == one["start"] and len(one["result"]["status"]) == 4
    far = MR.register_points(ctx, dev(va + F(50)), dev(v), dev(t), 0.4)                   # nothing in reach: no pose, no points
    assert far["R"] is None and far["points"] is None and far["result"]["status"].tolist() == [MR.FEW]


def test_mesh_compare_with_and_without_register(ctx, tmp_path):
    v, t, va, Rm, tm = moved_copy()
    a, b, c = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    nrm = np.tile(np.array([(0, 0, 1)], F), (len(va), 1))
    TS.write_mesh_ply(a, va, None, t, nrm)
    TS.write_mesh_ply(b, v, None, t)
    tool = [sys.executable, os.path.join(ROOT, "tools", "mesh_compare.py"), a, b, "--max-distance", "0.4"]
    plain = subprocess.run(tool, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    before = MD.mesh_deviation(ctx, dev(va), dev(t), dev(v), dev(t), 0.4)
    assert plain.stdout == (f"{a}: {len(va)} vertices, {len(t)} triangles; {b}: {len(v)} vertices, {len(t)} triangles; truncated at 0.4 m\n"
                            f"A -> B: {MD.summary_line(before['a_to_b'])}\nB -> A: {MD.summary_line(before['b_to_a'])}\n"
                            f"vertex-sampled symmetric Hausdorff distance, truncated: {before['hausdorff']:.6f} m\n")      # the bytes of the tool without the options
    got = MR.register_mesh(ctx, dev(va), dev(t), dev(v), dev(t), 0.4, "principal")
    r = subprocess.run(tool + ["--register", "--starts", "principal", "--out-aligned", c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(got["result"]["status"]) == 4 and got["after"]["a_to_b"]["rms"] < before["a_to_b"]["rms"] / 20
    for line in MR.pose_lines(got) + [f"before, A -> B: {MD.summary_line(before['a_to_b'])}", f"before, B -> A: {MD.summary_line(before['b_to_a'])}", "after:",
                                      f"A -> B: {MD.summary_line(got['after']['a_to_b'])}", f"B -> A: {MD.summary_line(got['after']['b_to_a'])}"]:
        assert line + "\n" in r.stdout, (line, r.stdout)
    with open(c, "rb") as f:
        cv, _, ct, cn = TS.read_mesh_ply(f.read())
    assert cv.tobytes() == got["points"].cpu().numpy().tobytes() and ct.tobytes() == t.astype(U32).tobytes()
    assert cn.tobytes() == RM.apply(pose_of(got["R"], got["t"]), va, nrm)[1].tobytes()


def test_track_dataset_with_and_without_register(ctx, tmp_path):
    """--mesh-reference alone prints what it printed before and writes the same files; with --mesh-reference-register the same files, the
    pose and the status, and the figures before (those of the run without it) and after"""
    from rgbid import synth
    from tests.test_gpu_cloud import K_SMALL, write_tum_folder
    rows, cols, n = 120, 160, 30                 # the sequence of the other command-line mesh tests: fewer frames export no keyframe
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    plain = str(tmp_path / "plain.ply")
    said = {}
    for name, extra in (("plain", []), ("own", ["--mesh-reference", plain]), ("registered", ["--mesh-reference", plain, "--mesh-reference-register"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply"), "--mesh-voxel", "0.04"] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = r.stdout
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "own.ply").read_bytes() == (tmp_path / "registered.ply").read_bytes()
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_own.txt").read_bytes() == (tmp_path / "traj_registered.txt").read_bytes()
    with open(plain, "rb") as f:
        v, _, t, *_ = TS.read_mesh_ply(f.read())
    assert len(t) > 0 and "mesh reference" not in said["plain"]
    own = MD.mesh_deviation(ctx, dev(v), dev(t), dev(v), dev(t), 0.16)                    # the volume's truncation distance: 4 voxels
    lines = [l.split(": ", 1)[1] for l in said["own"].splitlines() if "mesh reference" in l]
    assert lines == [f"mesh reference: written -> {plain}: {MD.summary_line(own['a_to_b'])}", f"mesh reference: {plain} -> written: {MD.summary_line(own['b_to_a'])}"]
    rest = lambda text: [l for l in text.splitlines() if "mesh reference" not in l and "frames/s" not in l]      # all but the timing line
    assert rest(said["own"]) == rest(said["registered"].replace("registered", "own"))      # the files' own names apart
    got = MR.register_mesh(ctx, dev(v), dev(t), dev(v), dev(t), 0.16)
    lines = [l.split(": ", 1)[1] for l in said["registered"].splitlines() if "mesh reference" in l]
    want = [f"mesh reference: {l}" for l in MR.pose_lines(got)]
    for word in ("before", "after"):
        want += [f"mesh reference ({word}): written -> {plain}: {MD.summary_line(got[word]['a_to_b'])}",
                 f"mesh reference ({word}): {plain} -> written: {MD.summary_line(got[word]['b_to_a'])}"]
    assert lines == want and got["before"] == own and got["status"] in ("converged", "running")
