"""GPU tests of the consistency filter (include/rgbid_consist.h, csrc/kernels_consist.hip, rgbid.consist): counts, kept count, statistics
and the emitted bytes against the numpy restatement (tests/consist_mirror.py) on a random cloud with the adversaries of the contract and
planes with every kind of hole, the same at 524 288, 524 289 and 1 053 579 records (one grid and 256 compaction tiles, one more, three
trips of the strided kernels) with one handle that also filters small clouds in between, the tolerance and the gates to the ulp, windows clipped at the image border, record order, the position
of a view in the batch, owner ranges, the refusals, the empty cloud, the cloud of a tracked run, and the options of
tools/track_dataset.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import cloud as CL
from rgbid import consist as CF
from rgbid import render as RD
from rgbid import sequence, synth, tum
from tests import consist_mirror as CM
from tests.test_cpu_consist import (COLS, HALF, K, LARGE_GATE, LARGE_N, ROWS, assert_every_trip_has_work, cameras, large_cloud, records_near_surface,
                                    surface_planes, unpack)
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GATE = dict(z_min=0.3, z_max=5.0)


def upload(p):
    return torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1, 32).copy()).cuda()


def finite(p):
    return np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])


def check(ctx, p, offsets, planes, R, t, K_=K, cf=None, dev=None, dplanes=None, **kw):
    """device filter of records p against the mirror: counts, kept, statistics, the emitted bytes and the kept offsets
    -> (support, conflicts, keep, plan)"""
    dev = upload(p) if dev is None else dev
    dplanes = torch.from_numpy(np.ascontiguousarray(planes, F)).cuda() if dplanes is None else dplanes
    rows, cols = dplanes.shape[-2:]
    own = cf is None
    cf = CF.ConsistencyFilter(ctx, max(len(p), 1), len(dplanes)) if own else cf
    res = cf.filter(dev, offsets, dplanes, R, t, K_, rows, cols, return_counts=True, return_offsets=offsets is not None, return_plan=True, **kw)
    if own:
        cf.close()
    out, cnt, plan = res[0], res[1], res[-1]
    ecnt, ekeep, ekept, epairs = CM.consist_numpy(p, offsets, planes, R, t, K_, **kw)
    got = cnt.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != ecnt)[0]
    assert bad.size == 0, (bad.size, bad[:5], [hex(v) for v in got[bad[:5]]], [hex(v) for v in ecnt[bad[:5]]], p[bad[:5]])
    sup, con = unpack(got)
    assert (plan.kept, plan.n, plan.finite, plan.pairs, plan.contradicted) == (int(ekeep.sum()), len(p), int(finite(p).sum()), epairs, int((con > 0).sum()))
    assert out.shape[0] == plan.kept and CL.as_numpy(out).tobytes() == ekept.tobytes()
    if offsets is not None:
        want = np.concatenate([[0], np.cumsum(ekeep)])[np.asarray(offsets, np.int64)]
        assert np.array_equal(res[2], want) and res[2].dtype == np.uint64
    return sup, con, ekeep, plan


_scenes = {}


def scene(V):
    """5 003 records (no multiple of 64 or 256) around a smooth surface that V cameras see, the planes with every kind of hole"""
    if V not in _scenes:
        rng = np.random.default_rng(100 + V)
        R, t = cameras(rng, V)
        planes = surface_planes(rng, R, t)
        p = records_near_surface(rng, 5003)
        p["y"][rng.random(len(p)) < 0.01] = -np.inf
        _scenes[V] = dict(p=p, R=R, t=t, planes=planes, dev=upload(p), dplanes=torch.from_numpy(planes).cuda())
    return _scenes[V]


@pytest.mark.parametrize("w", [0, 1, 2])
@pytest.mark.parametrize("V", [3, 19])
def test_consist_random_cloud(ctx, V, w):
    sc = scene(V)
    for kind in (np.nan, 0.0, -0.5, np.inf, 1e-39):
        assert (sc["planes"] == F(kind)).any() or (np.isnan(kind) and np.isnan(sc["planes"]).any())
    sup, con, keep, plan = check(ctx, sc["p"], None, sc["planes"], sc["R"], sc["t"], dev=sc["dev"], dplanes=sc["dplanes"], tol_rel=0.02, tol_abs=0.001,
                                 window=w, **GATE)
    assert sup.max() >= 2 and con.max() >= 2 and (sup > 0).sum() > 500 and (con > 0).sum() > 100 and 0 < plan.kept < plan.finite < plan.n
    assert plan.pairs > plan.n
    sup1, con1, keep1, plan1 = check(ctx, sc["p"], None, sc["planes"], sc["R"], sc["t"], dev=sc["dev"], dplanes=sc["dplanes"], tol_rel=0.02, tol_abs=0.001,
                                     window=w, min_support=2, max_conflicts=1, **GATE)
    assert np.array_equal(sup1, sup) and np.array_equal(con1, con) and 0 < plan1.kept != plan.kept


def test_consist_either_side_of_the_view_chunk(ctx):
    """exactly VIEW_CHUNK views go through the one launch that walks them all, one more through the chunked launches and the mark pass"""
    V = CF.VIEW_CHUNK + 1
    sc = scene(V)
    n = len(sc["p"])
    off = (np.arange(V + 1) * n // V).astype(np.uint64)
    for nv in (V - 1, V):
        o = off[:nv + 1].copy(); o[-1] = n
        check(ctx, sc["p"], o, sc["planes"][:nv], sc["R"][:nv], sc["t"][:nv], dev=sc["dev"], dplanes=sc["dplanes"][:nv], tol_rel=0.02, tol_abs=0.001,
              window=1, min_support=1, max_conflicts=1, **GATE)


# ---- past one grid of the strided kernels and one trip of the scan of the tile counts -------------------------------------------------
@pytest.fixture(scope="module")
def large(ctx):
    """large_cloud() on the device and the one handle every large case and the small clouds between them go through"""
    sc = dict(large_cloud())
    sc.update(dev=upload(sc["p"]), dplanes=torch.from_numpy(sc["planes"]).cuda(), cf=CF.ConsistencyFilter(ctx, LARGE_N, CF.VIEW_CHUNK + 1))
    yield sc
    sc["cf"].close()


def check_prefix(ctx, sc, n, V, offsets=None, **kw):
    """the first n records of the large cloud against its first V views, through the shared handle"""
    return check(ctx, sc["p"][:n], offsets, sc["planes"][:V], sc["R"][:V], sc["t"][:V], cf=sc["cf"], dev=sc["dev"][:n], dplanes=sc["dplanes"][:V],
                 **dict(LARGE_GATE, **kw))


@pytest.mark.parametrize("n", [HALF, HALF + 1, LARGE_N])
def test_consist_either_side_of_one_grid(ctx, large, n):
    """524 288 records: every thread makes one trip and k_vox_scan1 one; one record more: a second trip of one thread, a 257th tile;
    1 053 579: three trips, the lanes of the last wave make different numbers of them"""
    sup, con, keep, plan = check_prefix(ctx, large, n, 3)
    print(f"{n} records, 3 views: {plan.kept} kept, {int((sup > 0).sum())} supported, {plan.contradicted} contradicted, {plan.pairs} pairs")
    assert_every_trip_has_work(sup, con, keep, plan.pairs, n)


def test_consist_owner_range_across_the_second_trip(ctx, large):
    """the second view owns records 524 000 .. 524 599: the owner test on the first trip and on the second"""
    off = np.array([0, 524000, 524600, LARGE_N], np.uint64)
    free_sup, free_con, _, free = check_prefix(ctx, large, LARGE_N, 3)
    sup, con, keep, plan = check_prefix(ctx, large, LARGE_N, 3, off)
    assert_every_trip_has_work(sup, con, keep, plan.pairs, LARGE_N)
    own = slice(524000, 524600)
    assert plan.pairs < free.pairs and (sup <= free_sup).all() and (con <= free_con).all()
    assert (sup[own][:288] < free_sup[own][:288]).any() and (sup[own][288:] < free_sup[own][288:]).any()       # either side of record 524 288


def test_consist_one_handle_large_and_small_in_turn(ctx, large):
    """large, small, large in chunks of views, small in chunks: each equals its mirror, so no count, keep flag or tile offset of a larger
    plan is left in a smaller one.  The chunked large plan runs the memset of the counts, the integer adds of two chunks and the stride
    of k_consist_mark past one grid, with owner ranges"""
    V = CF.VIEW_CHUNK + 1
    vote = dict(min_support=1, max_conflicts=1)

    def small(views):
        sc = scene(3 if views == 3 else 19)               # 5 003 records; the handle holds VIEW_CHUNK + 1 views
        return check(ctx, sc["p"], None, sc["planes"][:views], sc["R"][:views], sc["t"][:views], cf=large["cf"], dev=sc["dev"],
                     dplanes=sc["dplanes"][:views], tol_rel=0.02, tol_abs=0.001, window=1, **GATE, **(vote if views > 3 else {}))
    check_prefix(ctx, large, LARGE_N, 3)
    sup, con, _, plan = small(3)
    assert (sup > 0).sum() > 500 and (con > 0).sum() > 100 and 0 < plan.kept < plan.n
    n = HALF + 5003
    off = (np.arange(V + 1, dtype=np.uint64) * np.uint64(n) // np.uint64(V)).astype(np.uint64)
    sup, con, keep, plan = check_prefix(ctx, large, n, V, off, **vote)
    print(f"{n} records, {V} views: {plan.kept} kept, {int((sup > 0).sum())} supported, {plan.contradicted} contradicted, {plan.pairs} pairs")
    assert sup.max() > 3 and (con[HALF:] > 1).any() and (~keep[HALF:]).sum() > 100 and keep[HALF:].sum() > 100
    sup, con, _, plan = small(V)
    assert (sup > 0).sum() > 500 and (con > 0).sum() > 100 and 0 < plan.kept < plan.n


# ---- the tolerance and the gates to the ulp -----------------------------------------------------------------------------------------
def on_axis(zs):
    p = np.zeros(len(zs), CL.POINT_DTYPE)
    p["z"] = zs
    p["r"] = np.arange(len(zs))
    return p


def test_consist_boundaries_to_the_ulp(ctx):
    """the identity camera before a wall at 2 m (iD = 0.5), records on its axis.  tol_abs = 0.25, tol_rel = 0: at Z = 1.75 e = d exactly:
    support; one ulp nearer e > d: contradiction; at Z = 2.25 |e| = d: support; one ulp farther: blind.  Every e here is exact.  With
    tol_rel = 0.125: d = 0.125 Z is exact too, and e = d at Z = 16 / 9 has no float, so the mirror alone judges the neighbours of it.
    A wall at 8 m contradicts whatever passes the gate: Z on each gate does, one ulp outside does not."""
    R, t = np.eye(3)[None], np.zeros((1, 3))
    wall = np.full((1, ROWS, COLS), 0.5, F)
    lo, hi = F(1.75), F(2.25)
    zs = [lo, np.nextafter(lo, F(0)), np.nextafter(lo, F(9)), hi, np.nextafter(hi, F(0)), np.nextafter(hi, F(9))]
    for w in (0, 2):
        sup, con, _, _ = check(ctx, on_axis(zs), None, wall, R, t, tol_rel=0.0, tol_abs=0.25, window=w, **GATE)
        assert sup.tolist() == [1, 0, 1, 1, 1, 0] and con.tolist() == [0, 1, 0, 0, 0, 0]
    z0 = F(16.0 / 9.0)
    near = [z0]
    for _ in range(3):
        near = [np.nextafter(near[0], F(0))] + near + [np.nextafter(near[-1], F(9))]
    sup, con, _, _ = check(ctx, on_axis(near), None, wall, R, t, tol_rel=0.125, tol_abs=0.0, window=0, **GATE)
    assert sup[-1] == 1 and con[0] == 1 and (sup + con == 1).all() and (np.diff(sup) >= 0).all()
    far = np.full((1, ROWS, COLS), 0.125, F)
    zmin, zmax = F(0.3), F(5.0)
    zs = [zmin, np.nextafter(zmin, F(0)), np.nextafter(zmin, F(9)), zmax, np.nextafter(zmax, F(0)), np.nextafter(zmax, F(9))]
    sup, con, _, plan = check(ctx, on_axis(zs), None, far, R, t, tol_rel=0.02, tol_abs=0.0, window=1, **GATE)
    assert con.tolist() == [1, 0, 1, 1, 1, 0] and not sup.any() and plan.pairs == 4


# ---- windows at the image border ----------------------------------------------------------------------------------------------------
K_CORNER = (64.0, 32.0, 0.0, 0.0)       # powers of two and the principal point in the corner: u = 64 x at Z = 1 is exact


def test_consist_window_clipped_at_the_border(ctx):
    """records at Z = 1 that project onto the corners, the edges and one pixel inside them, w = 2: the 5 x 5 window is clipped to 3 x 3 in a
    corner.  A plane that is a hole everywhere but at one far pixel: the records whose clipped window holds that pixel are contradicted,
    the others are blind -- a window that wrapped round a row end, or was not clipped, would count differently.  Then a random plane with
    holes against the mirror."""
    us = [0, 1, 2, 3, COLS - 4, COLS - 3, COLS - 2, COLS - 1]
    vs = [0, 1, 2, 3, ROWS - 4, ROWS - 3, ROWS - 2, ROWS - 1]
    uv = np.array([(u, v) for v in vs for u in us])
    p = on_axis(np.ones(len(uv), F))
    p["x"], p["y"] = (uv[:, 0] / 64).astype(F), (uv[:, 1] / 32).astype(F)
    R, t = np.eye(3)[None], np.zeros((1, 3))
    for px, py in ((0, 0), (COLS - 1, ROWS - 1), (COLS - 1, 0), (2, ROWS - 1), (COLS - 1, 1)):
        plane = np.full((1, ROWS, COLS), np.nan, F)
        plane[0, py, px] = 0.25
        sup, con, _, _ = check(ctx, p, None, plane, R, t, K_CORNER, tol_rel=0.02, tol_abs=0.0, window=2, **GATE)
        near = (np.abs(uv[:, 0] - px) <= 2) & (np.abs(uv[:, 1] - py) <= 2)
        assert np.array_equal(con == 1, near) and not sup.any() and near.sum() >= 9
    rng = np.random.default_rng(7)
    plane = rng.choice(np.array([0.5, 1.0, 0.99, 2.0, np.nan, 0.0, np.inf], F), (1, ROWS, COLS))
    for w in (1, 2):
        sup, con, _, _ = check(ctx, p, None, plane, R, t, K_CORNER, tol_rel=0.02, tol_abs=0.0, window=w, **GATE)
        assert sup.sum() > 20


# ---- order ----------------------------------------------------------------------------------------------------------------------------
def test_consist_permuting_the_records_permutes_the_counts(ctx):
    sc = scene(3)
    kw = dict(tol_rel=0.02, tol_abs=0.001, window=1, **GATE)
    sup, con, keep, _ = check(ctx, sc["p"], None, sc["planes"], sc["R"], sc["t"], dev=sc["dev"], dplanes=sc["dplanes"], **kw)
    perm = np.random.default_rng(23).permutation(len(sc["p"]))
    psup, pcon, pkeep, _ = check(ctx, sc["p"][perm], None, sc["planes"], sc["R"], sc["t"], dplanes=sc["dplanes"], **kw)
    assert np.array_equal(psup, sup[perm]) and np.array_equal(pcon, con[perm]) and np.array_equal(pkeep, keep[perm])


def test_consist_view_order_changes_nothing(ctx):
    """19 views: the first one moved to place 17 and the last one to the front leave every count as it was"""
    sc = scene(19)
    kw = dict(tol_rel=0.02, tol_abs=0.001, window=1, **GATE)
    sup, con, _, plan = check(ctx, sc["p"], None, sc["planes"], sc["R"], sc["t"], dev=sc["dev"], dplanes=sc["dplanes"], **kw)
    order = [18] + list(range(1, 17)) + [0, 17]
    assert sorted(order) == list(range(19))
    osup, ocon, _, oplan = check(ctx, sc["p"], None, sc["planes"][order], sc["R"][order], sc["t"][order], dev=sc["dev"], **kw)
    assert np.array_equal(osup, sup) and np.array_equal(ocon, con) and oplan.pairs == plan.pairs


@pytest.mark.parametrize("V", [3, 19])
def test_consist_owner_exclusion(ctx, V):
    """real offsets, an empty owner range among them: a view is no witness of its own records, and the counts of the others' are unchanged"""
    sc = scene(V)
    n = len(sc["p"])
    kw = dict(tol_rel=0.02, tol_abs=0.001, window=1, **GATE)
    cuts = np.sort(np.random.default_rng(V).integers(0, n + 1, V - 1))
    cuts[1] = cuts[0]                                       # view 1 owns nothing
    off = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    free_sup, free_con, _, free = check(ctx, sc["p"], None, sc["planes"], sc["R"], sc["t"], dev=sc["dev"], dplanes=sc["dplanes"], **kw)
    sup, con, _, plan = check(ctx, sc["p"], off, sc["planes"], sc["R"], sc["t"], dev=sc["dev"], dplanes=sc["dplanes"], **kw)
    assert plan.pairs < free.pairs and (sup <= free_sup).all() and (con <= free_con).all() and (sup < free_sup).any()
    assert (free_sup - sup <= 1).all() and (free_con - con <= 1).all()


# ---- refusals and edge cases ----------------------------------------------------------------------------------------------------------
def test_consist_refusals_and_reuse(ctx):
    rng = np.random.default_rng(37)
    V, n = 2, 300
    R, t = cameras(rng, V)
    planes = surface_planes(rng, R, t)
    p = records_near_surface(rng, n)
    dev, dplanes = upload(p), torch.from_numpy(planes).cuda()
    off = np.array([0, 100, n], np.uint64)
    cf = CF.ConsistencyFilter(ctx, n, V)
    L = cf.L
    kept = C.c_ulonglong()
    kw = dict(tol_rel=0.02, tol_abs=0.001, window=1, **GATE)

    def call(**ch):
        a = dict(ptr=dev.data_ptr(), n=n, V=V, R=R, t=t, planes=[dplanes[v].data_ptr() for v in range(V)], off=off, K=K, rows=ROWS, cols=COLS,
                 tol_rel=0.02, tol_abs=0.001, window=1, z_min=0.3, z_max=5.0, min_support=0, max_conflicts=0)
        a.update(ch)
        views = (CF.View * max(a["V"], 1))(*[CF.View(RD.Pose((C.c_double * 9)(*np.asarray(a["R"][v % V], np.float64).reshape(9)),
                                                             (C.c_double * 3)(*np.asarray(a["t"][v % V], np.float64))), a["planes"][v % V])
                                             for v in range(max(a["V"], 1))])
        prm = CF.Params(a["tol_rel"], a["tol_abs"], a["window"], a["z_min"], a["z_max"], a["min_support"], a["max_conflicts"])
        o = None if a["off"] is None else np.ascontiguousarray(a["off"], np.uint64)
        return L.rgbid_consist_plan(cf._h, C.c_void_p(a["ptr"]), C.c_ulonglong(a["n"]), a["V"], views, None if o is None else o.ctypes.data_as(C.c_void_p),
                                    (C.c_float * 4)(*a["K"]), a["rows"], a["cols"], C.byref(prm), None, C.byref(kept))

    def still_works():
        _, _, _, plan = check(ctx, p, off, planes, R, t, cf=cf, dev=dev, dplanes=dplanes, **kw)
        assert 0 < plan.kept < n
        return plan

    still_works()
    nan, inf = float("nan"), float("inf")
    Rn = R.copy(); Rn[1, 0, 1] = nan
    ti = t.copy(); ti[0, 2] = inf
    tb = t.copy(); tb[1, 0] = 1e300                      # finite as a double, infinite as the float the device would get
    p0, p1 = dplanes[0].data_ptr(), dplanes[1].data_ptr()
    refusals = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(cols=(1 << 20) + 1), dict(V=0), dict(V=3, off=None), dict(n=n + 1, off=None),
                dict(window=-1), dict(window=3), dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=nan), dict(z_max=nan), dict(z_max=inf),
                dict(z_min=2.0, z_max=1.0), dict(tol_rel=-0.01), dict(tol_rel=nan), dict(tol_rel=inf), dict(tol_abs=-1e-3), dict(tol_abs=nan),
                dict(tol_abs=inf), dict(min_support=65536), dict(max_conflicts=65536), dict(R=Rn), dict(t=ti), dict(t=tb),
                dict(K=(nan, 58.0, 31.5, 23.5)), dict(K=(60.0, 58.0, inf, 23.5)), dict(K=(0.0, 58.0, 31.5, 23.5)), dict(K=(60.0, 0.0, 31.5, 23.5)),
                dict(planes=[p0, 0]), dict(planes=[p0 + 2, p1]), dict(ptr=dev.data_ptr() + 8, n=n - 1, off=None), dict(ptr=0),
                dict(off=[1, 100, n]), dict(off=[0, 200, 100]), dict(off=[0, 100, n - 1]), dict(off=[0, 100, n + 1])]
    for ch in refusals:
        assert call(**ch) == -1, ch
    still_works()
    for ch in (dict(rows=0), dict(window=3), dict(off=[0, 200, 100])):   # the handle is usable after each kind of refusal, not only after all
        assert call(**ch) == -1, ch
        still_works()
    assert call() == 0 and call(off=None) == 0 and call(ptr=0, n=0, off=[0, 0, 0]) == 0 and kept.value == 0
    for bad in (dict(tol_rel=-1), dict(window=3), dict(z_min=0), dict(R=Rn), dict(K=(0, 1, 1, 1)), dict(min_support=-1), dict(offsets=[0, 5, 2])):
        a = dict(offsets=off, planes=dplanes, R=R, t=t, K=K, rows=ROWS, cols=COLS)
        a.update(bad)
        with pytest.raises(ValueError):                   # the Python checks come first
            cf.plan(dev, **a)
    with pytest.raises(ValueError):
        cf.plan(dev, off, dplanes[:, :, :COLS - 1].contiguous(), R, t, K, ROWS, COLS)
    with pytest.raises(ValueError):
        cf.filter(dev, None, dplanes, R, t, K, ROWS, COLS, return_offsets=True)
    plan = still_works()
    canary = torch.full((plan.kept + 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.wait_torch_stream()
    with pytest.raises(Exception, match="rgbid error -1"):
        cf.emit(canary[:plan.kept - 1])                    # capacity below the plan's kept
    ctx.sync()
    assert (canary == 0xA5).all()
    cf.emit(canary[:plan.kept])                            # exactly kept: the record after them stays untouched
    ctx.sync()
    assert (canary[plan.kept] == 0xA5).all()
    assert CL.as_numpy(canary[:plan.kept]).tobytes() == CM.consist_numpy(p, off, planes, R, t, K, **kw)[2].tobytes()
    cf.timing(True)
    still_works()
    ms = cf.timing(False)
    print("consistency filter stage ms:", ms)
    assert tuple(ms) == CF.STAGES and all(np.isfinite(v) and v >= 0 for v in ms.values()) and sum(ms.values()) > 0
    cf.close()
    for mp, mv in ((0, 2), (1 << 31, 2), (10, 0), (10, 65536)):
        with pytest.raises(Exception):
            CF.ConsistencyFilter(ctx, mp, mv)


def test_consist_empty_and_nothing_finite(ctx):
    sc = scene(3)
    out, cnt, off, plan = CF.consistency_filter(ctx, sc["dev"][:0], [0, 0, 0, 0], sc["dplanes"], sc["R"], sc["t"], K, ROWS, COLS, return_counts=True,
                                                return_offsets=True, return_plan=True)
    assert out.shape == (0, 32) and cnt.shape == (0,) and off.tolist() == [0, 0, 0, 0] and (plan.kept, plan.n, plan.pairs) == (0, 0, 0)
    q = sc["p"][:200].copy()
    q["x"] = np.nan
    sup, con, keep, plan = check(ctx, q, None, sc["planes"], sc["R"], sc["t"], dplanes=sc["dplanes"], **GATE)
    assert plan.finite == 0 and plan.kept == 0 and not sup.any() and not con.any()


# ---- a tracked run and the command line -----------------------------------------------------------------------------------------------
_run = {}


def tracked_run(ctx, tmp_path_factory):
    """the small synthetic TUM folder of tests/test_gpu_cloud.py, read back and tracked in two chunks with the keyframes' depth kept: once
    as tools/track_dataset.py tracks it (`pc`), once with the keyframe thresholds of tests/test_gpu_render.py, which export more
    keyframes (`pc_many`)"""
    if not _run:
        rows, cols, n = 120, 160, 30
        seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
        root = tmp_path_factory.mktemp("consist") / "synth"
        write_tum_folder(root, seq)
        gs = tum.Dataset(str(root))
        frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
        gs.close()
        depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
        rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
        _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True)
        _, _, _, many = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True, visratio_odo=0.985,
                                               visratio_integr=0.97)
        _run.update(root=root, rows=rows, cols=cols, pc=pc, pc_many=many)
    return _run


def test_consist_on_a_tracked_run(ctx, tmp_path_factory):
    run = tracked_run(ctx, tmp_path_factory)
    pc, rows, cols = run["pc_many"], run["rows"], run["cols"]
    kfs = pc.keyframes
    assert len(kfs) >= 3 and len(pc) > 10_000
    R, t = np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs])
    dplanes = torch.stack([k["depthinv"] for k in kfs])
    planes = dplanes.cpu().numpy()
    for kw in (dict(), dict(tol_rel=0.01, tol_abs=0.002, window=2, min_support=1, max_conflicts=1)):
        sup, con, keep, plan = check(ctx, pc.numpy(), pc.offsets, planes, R, t, K_SMALL, dev=pc.points, dplanes=dplanes, **kw)
        print(f"tracked run: {plan.n} records of {len(kfs)} keyframes, {kw or 'defaults'}: {plan.kept} kept, {plan.contradicted} contradicted, "
              f"{int((sup > 0).sum())} supported, {plan.pairs} pairs past the gates")
        assert (sup > 0).sum() > 0 and plan.pairs > 0
    kept, off = CF.consistency_filter(ctx, pc.points, pc.offsets, [k["depthinv"] for k in kfs], R, t, K_SMALL, rows, cols, return_offsets=True)
    assert int(off[-1]) == kept.shape[0] and len(off) == len(kfs) + 1
    figures = RD.depth_agreement(ctx, kept, off, kfs, K_SMALL, rows, cols, 1)      # the filtered cloud still knows its keyframes
    assert len(figures) == len(kfs)


def test_track_dataset_consistency_options(ctx, tmp_path, tmp_path_factory):
    """without the new options the PLY and the trajectory are what they were: the cloud of the same run in process; with
    --cloud-consistency the PLY holds exactly the library's kept records and the trajectory is unchanged"""
    run = tracked_run(ctx, tmp_path_factory)
    pc, rows, cols = run["pc"], run["rows"], run["cols"]
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(run["root"]), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("consist", ["--cloud-consistency", "0.02", "--render-check"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--cloud", str(tmp_path / f"{name}.ply")] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = r.stdout
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_consist.txt").read_bytes()
    assert (tmp_path / "plain.ply").read_bytes() == CL.ply_bytes(pc.points)
    kfs = pc.keyframes
    kept, plan = CF.consistency_filter(ctx, pc.points, pc.offsets, [k["depthinv"] for k in kfs], np.stack([k["R"] for k in kfs]),
                                       np.stack([k["t"] for k in kfs]), K_SMALL, rows, cols, tol_rel=0.02, return_plan=True)
    assert (tmp_path / "consist.ply").read_bytes() == CL.ply_bytes(kept) and 0 < plan.kept <= plan.n
    assert f"{plan.kept} kept, {plan.n - plan.kept} removed, {plan.contradicted} contradicted" in said["consist"], said["consist"]
    assert " contradicted (" not in said["plain"] and "after the consistency filter" not in said["plain"]
    assert f"render check after the consistency filter: {len(kfs)} keyframes" in said["consist"]
    assert len(re.findall(r"render check after the consistency filter: keyframe at frame \d+: \d+ pixels", said["consist"])) == len(kfs)
