"""GPU tests of the map renderer (include/rgbid_render.h, csrc/kernels_render.hip, rgbid.render): every plane against the bytes of the numpy
restatement (tests/render_mirror.py) on a random cloud with the adversaries of the contract, ties, the image borders to the ulp, record
order, the position of a view in a batch across the per-launch view chunk, contention on one pixel block, the refusals, and the cloud of
a tracked run with the depth agreement figures."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import cloud as CL
from rgbid import render as RD
from rgbid import sequence, synth, tum
from tests import render_mirror as RM
from tests.test_cpu_render import cloud_around, rotation
from tests.test_cpu_voxel import random_cloud
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ROWS, COLS = 48, 64
K = (60.0, 58.0, 31.5, 23.5)
Z_MIN, Z_MAX = 0.3, 2.5
ALL = ("index", "depth", "colour", "normal")


def upload(p):
    return torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1, 32).copy()).cuda()


def bits(name, a):
    """a plane as the integers that are compared: float planes as uint32, so that NaN patterns count"""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if name != "colour" else a


def assert_planes(got, want, what=""):
    for name in want:
        g, w = bits(name, got[name]), bits(name, want[name])
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:4].tolist(), [(g[tuple(b)], w[tuple(b)]) for b in bad[:4]])


def check(ctx, p, R, t, K_, rows, cols, s, z_min=Z_MIN, z_max=Z_MAX, rd=None, dev=None, want=None):
    """device rendering of records p against the mirror, all four planes -> (device planes as numpy, mirror planes)"""
    dev = upload(p) if dev is None else dev
    if rd is None:
        got = RD.render_views(ctx, dev, R, t, K_, rows, cols, s, z_min, z_max, ALL)
    else:
        got = rd.render(dev, R, t, K_, rows, cols, s, z_min, z_max, ALL)
    want = RM.render_numpy(p, R, t, K_, rows, cols, s, z_min, z_max) if want is None else want
    assert_planes(got, want, f"s={s}")
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got["index"] = got["index"].view(np.uint32)          # the tensor is int32: -1 is EMPTY
    return got, want


def three_cameras(rng):
    """one at the origin looking along +z with the identity pose (Z = z exactly), two moved and turned"""
    R = np.stack([np.eye(3), rotation(rng, 0.5), rotation(rng, 0.9)])
    t = np.stack([np.zeros(3), rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.6, 0.6, 3)])
    return R, t


def random_scene():
    rng = np.random.default_rng(17)
    n = 5003                                              # no multiple of 64 or 256
    p = cloud_around(rng, n)                              # in front of, beside and behind the cameras; NaN x, inf z, NaN ny
    p["y"][rng.random(n) < 0.01] = -np.inf
    p["nx"][rng.random(n) < 0.05] = np.inf                # inf * 0 and inf - inf in the rotated normal
    p["nz"][rng.random(n) < 0.05] = np.nan
    zs = [F(Z_MIN), np.nextafter(F(Z_MIN), F(0)), np.nextafter(F(Z_MIN), F(1)), F(Z_MAX), np.nextafter(F(Z_MAX), F(0)), np.nextafter(F(Z_MAX), F(9))]
    for k, z in enumerate(zs):                            # on the gate and one ulp either side of it, seen by the identity camera
        p["x"][k], p["y"][k], p["z"][k] = F(0.01 * k) * z, F(0), z
    R, t = three_cameras(rng)
    return p, R, t


_scene = {}


def scene():
    if not _scene:
        p, R, t = random_scene()
        _scene.update(p=p, R=R, t=t, dev=None)
    return _scene


@pytest.mark.parametrize("s", [0, 1, 4])
def test_render_random_cloud(ctx, s):
    sc = scene()
    p, R, t = sc["p"], sc["R"], sc["t"]
    got, want = check(ctx, p, R, t, K, ROWS, COLS, s)
    hit = want["index"] != RM.EMPTY
    assert (hit.reshape(3, -1).sum(1) > 100).all() and (s == 4 or not hit.all())
    i, _, _, Z = RM.visible(p, RM.pose_cw(R[0], t[0]), K, ROWS, COLS, s, Z_MIN, Z_MAX)
    assert {0, 2, 3, 4} <= set(i.tolist()) and not {1, 5} & set(i.tolist())       # on the gate and inside stay, one ulp outside goes
    assert Z[i == 0][0] == F(Z_MIN) and Z[i == 3][0] == F(Z_MAX)
    nanbits = got["normal"].view(np.uint32) == RM.NAN_BITS
    assert (nanbits[np.broadcast_to(hit[:, None], nanbits.shape)]).any()           # a winner with a NaN normal was drawn
    assert not (np.isnan(got["normal"]) & ~nanbits).any()


def test_render_ties_go_to_the_smallest_index(ctx):
    rng = np.random.default_rng(5)
    p = cloud_around(rng, 200, nan=0.0)
    p["z"] += F(1.5)                                      # the crowd lies behind the tied records
    tied = [7, 50, 51, 120, 199]
    for k in tied:
        p["x"][k], p["y"][k], p["z"][k] = F(0.1), F(0.05), F(1.0)
    p["r"] = np.arange(200)
    R, t = np.eye(3)[None], np.zeros((1, 3))
    got, _ = check(ctx, p, R, t, K, ROWS, COLS, 1, 0.3, 5.0)
    pu, pv = int(np.floor(F(60) * F(0.1) + F(31.5) + F(0.5))), int(np.floor(F(58) * F(0.05) + F(23.5) + F(0.5)))
    assert got["index"][0, pv, pu] == 7 and got["colour"][0, pv, pu, 0] == 7 and got["depth"][0, pv, pu] == 1.0
    q = p[::-1].copy()
    rev, _ = check(ctx, q, R, t, K, ROWS, COLS, 1, 0.3, 5.0)
    assert rev["index"][0, pv, pu] == 0 and rev["colour"][0, pv, pu, 0] == 199    # record 199 is now record 0
    assert np.array_equal(rev["depth"].view(np.uint32), got["depth"].view(np.uint32))


# ---- borders ------------------------------------------------------------------------------------------------------------------------
K_CORNER = (64.0, 32.0, 0.0, 0.0)     # powers of two and the principal point in the corner: u = 64 x / 1 + 0 is exact, so u takes every float


def border_records(axis):
    """eight records at Z = 1 whose u (axis 0) or v (axis 1) is: -0.5 (u + 0.5 lands at 0), one ulp below, one ulp above; size - 0.5 (lands at
    size), one ulp below, one ulp above; size + 1 (p = size - 1 + 2) and size + 2 (p = size + 2).  Each on a row (column) of its own, 6 apart."""
    size, f = (COLS, F(64)) if axis == 0 else (ROWS, F(32))
    lo, hi = F(-0.5), F(size - 0.5)
    us = [lo, np.nextafter(lo, F(-9)), np.nextafter(lo, F(9)), hi, np.nextafter(hi, F(0)), np.nextafter(hi, F(99)), F(size + 1), F(size + 2)]
    p = np.zeros(8, CL.POINT_DTYPE)
    along, across = ("x", "y") if axis == 0 else ("y", "x")
    fa = F(32) if axis == 0 else F(64)
    for k, u in enumerate(us):
        p[along][k] = u / f                               # exact: a power of two
        p[across][k] = F(3 + 6 * k) / fa
        assert p[along][k] * f == u
    p["z"] = 1
    p["r"] = 10 + np.arange(8)
    return p, us


@pytest.mark.parametrize("axis", [0, 1])
def test_render_borders_to_the_ulp(ctx, axis):
    p, us = border_records(axis)
    assert us[1] < us[0] < us[2] and np.floor(us[1] + F(0.5)) == -1 and np.floor(us[0] + F(0.5)) == 0 and np.floor(us[2] + F(0.5)) == 0
    size = COLS if axis == 0 else ROWS
    assert np.floor(us[3] + F(0.5)) == size and np.floor(us[4] + F(0.5)) == size - 1 and np.floor(us[5] + F(0.5)) == size
    R, t = np.eye(3)[None], np.zeros((1, 3))
    for s, seen in ((0, {0, 2, 4}), (2, {0, 1, 2, 3, 4, 5, 6})):
        got, _ = check(ctx, p, R, t, K_CORNER, ROWS, COLS, s, 0.5, 2.0)
        idx = got["index"][0] if axis == 0 else got["index"][0].T          # [across, along]
        assert set(idx[idx != RM.EMPTY].tolist()) == seen, (s, set(idx[idx != RM.EMPTY].tolist()))
        for k in seen:                                    # each record paints the clipped square around its pixel and nothing else
            pa, pc = int(np.floor(us[k] + F(0.5))), 3 + 6 * k
            a0, a1 = max(pa - s, 0), min(pa + s, size - 1)
            where = np.argwhere(idx == k)
            assert where[:, 1].min() == a0 and where[:, 1].max() == a1 and where[:, 0].min() == pc - s and where[:, 0].max() == pc + s, (s, k)
            assert len(where) == (a1 - a0 + 1) * (2 * s + 1)
    got, _ = check(ctx, p, R, t, K_CORNER, ROWS, COLS, 2, 0.5, 2.0)
    idx = got["index"][0] if axis == 0 else got["index"][0].T
    assert (idx[:, size - 1] == 6).sum() == 5 and not (idx == 7).any()    # p = size - 1 + s still paints the last column; p = size + s nothing


# ---- order, batch, contention -------------------------------------------------------------------------------------------------------
def test_render_does_not_depend_on_record_order(ctx):
    sc = scene()
    R, t = sc["R"], sc["t"]
    rng = np.random.default_rng(23)
    p = cloud_around(rng, 3001, nan=0.0)
    for v in range(3):                                    # distinct Z among the visible records of every view: no tie to break by index
        i, _, _, Z = RM.visible(p, RM.pose_cw(R[v], t[v]), K, ROWS, COLS, 1, Z_MIN, Z_MAX)
        assert len(np.unique(Z)) == len(Z) > 300
    perm = rng.permutation(len(p))
    a, _ = check(ctx, p, R, t, K, ROWS, COLS, 1)
    b, _ = check(ctx, p[perm], R, t, K, ROWS, COLS, 1)
    for name in ("depth", "colour", "normal"):
        assert np.array_equal(bits(name, a[name]), bits(name, b[name])), name
    hit = a["index"] != RM.EMPTY
    assert np.array_equal(hit, b["index"] != RM.EMPTY) and np.array_equal(perm[b["index"][hit]], a["index"][hit])


def test_render_view_does_not_depend_on_its_place_in_the_batch(ctx):
    """33 views = two full launches of the per-launch view chunk and one more: the first view, the last of the first chunk, the first of
    the second chunk and the final view each equal the same view rendered alone (and the mirror)"""
    chunk = RD.VIEW_CHUNK
    V = 2 * chunk + 1
    rng = np.random.default_rng(29)
    p = scene()["p"]
    dev = upload(p)
    R = np.stack([rotation(rng, 0.6) for _ in range(V)])
    t = rng.uniform(-0.5, 0.5, (V, 3))
    rd = RD.Renderer(ctx, len(p), ROWS * COLS * V)
    batch = {k: v.cpu().numpy() for k, v in rd.render(dev, R, t, K, ROWS, COLS, 1, Z_MIN, Z_MAX, ALL).items()}
    for v in (0, chunk - 1, chunk, V - 1):
        alone, want = check(ctx, p, R[v:v + 1], t[v:v + 1], K, ROWS, COLS, 1, rd=rd, dev=dev)
        assert (want["index"] != RM.EMPTY).sum() > 100
        for name in ALL:
            assert np.array_equal(bits(name, batch[name][v]), bits(name, alone[name][0])), (v, name)
    rd.close()


def test_render_contention_on_one_pixel_block(ctx):
    """4 096 records of distinct Z that all project into the 2 x 2 block (10..11, 7..8): the early-out load and the atomic together must
    leave the global minimum of each pixel (s = 0) and of the block (s = 1: the squares overlap)"""
    rng = np.random.default_rng(31)
    n = 4096
    z = (F(0.5) + F(1e-4) * rng.permutation(n).astype(F)).astype(F)
    assert len(np.unique(z)) == n
    a, b = rng.integers(10, 12, n), rng.integers(7, 9, n)
    p = random_cloud(rng, n, nan=0.0)
    p["x"] = (F(1) / F(K[0]) * (a.astype(F) - F(K[2]))) * z
    p["y"] = (F(1) / F(K[1]) * (b.astype(F) - F(K[3]))) * z
    p["z"] = z
    R, t = np.eye(3)[None], np.zeros((1, 3))
    i, pu, pv, Z = RM.visible(p, RM.pose_cw(R[0], t[0]), K, ROWS, COLS, 0, Z_MIN, Z_MAX)
    assert len(i) == n and np.array_equal(pu, a) and np.array_equal(pv, b)
    dev = upload(p)
    got, _ = check(ctx, p, R, t, K, ROWS, COLS, 0, dev=dev)
    for y in (7, 8):
        for x in (10, 11):
            m = (a == x) & (b == y)
            assert got["index"][0, y, x] == np.nonzero(m)[0][np.argmin(z[m])] and got["depth"][0, y, x] == z[m].min()
    assert (got["index"][0] != RM.EMPTY).sum() == 4
    got, _ = check(ctx, p, R, t, K, ROWS, COLS, 1, dev=dev)
    assert (got["index"][0, 7:9, 10:12] == np.argmin(z)).all() and (got["index"][0] != RM.EMPTY).sum() == 16


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_render_refusals_and_reuse(ctx):
    rng = np.random.default_rng(37)
    rows, cols, n = 12, 16, 200
    Kt = (14.0, 13.0, 7.5, 5.5)
    p = cloud_around(rng, n)
    dev = upload(p)
    R, t = np.stack([np.eye(3), rotation(rng, 0.3)]), np.stack([np.zeros(3), rng.uniform(-0.2, 0.2, 3)])
    want = RM.render_numpy(p, R, t, Kt, rows, cols, 1, Z_MIN, Z_MAX)
    assert (want["index"] != RM.EMPTY).sum() > 40
    rd = RD.Renderer(ctx, n, rows * cols * 2)
    L = rd.L
    out = torch.empty((2, rows, cols), dtype=torch.float32, device="cuda")

    def call(**kw):
        a = dict(ptr=dev.data_ptr(), n=n, V=2, R=R, t=t, K=Kt, rows=rows, cols=cols, s=1, z_min=Z_MIN, z_max=Z_MAX)
        a.update(kw)
        poses = (RD.Pose * a["V"])(*[RD.Pose((C.c_double * 9)(*np.asarray(a["R"][v % 2], np.float64).reshape(9)),
                                             (C.c_double * 3)(*np.asarray(a["t"][v % 2], np.float64))) for v in range(a["V"])])
        return L.rgbid_render_views(rd._h, C.c_void_p(a["ptr"]), C.c_ulonglong(a["n"]), a["V"], poses, (C.c_float * 4)(*a["K"]), a["rows"], a["cols"],
                                    a["s"], C.c_float(a["z_min"]), C.c_float(a["z_max"]), None, C.c_void_p(out.data_ptr()), None, None)

    def still_works():
        check(ctx, p, R, t, Kt, rows, cols, 1, rd=rd, dev=dev, want=want)

    still_works()
    nan, inf = float("nan"), float("inf")
    Rn = R.copy(); Rn[1, 0, 1] = nan
    ti = t.copy(); ti[0, 2] = inf
    tb = t.copy(); tb[1, 0] = 1e300                      # finite as a double, infinite as the float the device would get
    refusals = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(V=3), dict(rows=2 * rows + 1), dict(V=0), dict(s=-1), dict(s=RD.MAX_SPLAT + 1),
                dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=nan), dict(z_max=nan), dict(z_max=inf), dict(z_min=inf, z_max=inf),
                dict(z_min=2.0, z_max=1.0), dict(R=Rn), dict(t=ti), dict(t=tb), dict(K=(nan, 13.0, 7.5, 5.5)), dict(K=(14.0, 13.0, inf, 5.5)),
                dict(K=(0.0, 13.0, 7.5, 5.5)), dict(K=(14.0, 0.0, 7.5, 5.5)), dict(n=n + 1), dict(ptr=dev.data_ptr() + 8, n=n - 1), dict(ptr=0)]
    for kw in refusals:
        assert call(**kw) == -1, kw
        still_works()
    assert call() == 0 and call(ptr=0, n=0) == 0
    for bad in (dict(rows=0), dict(splat=5), dict(z_min=0), dict(R=Rn), dict(K=(0, 1, 1, 1))):      # the Python checks come first
        a = dict(R=R, t=t, K=Kt, rows=rows, cols=cols, splat=1, z_min=Z_MIN, z_max=Z_MAX)
        a.update(bad)
        with pytest.raises(ValueError):
            rd.render(dev, **a)
    still_works()
    empty = rd.render(dev[:0], R, t, Kt, rows, cols, 1, Z_MIN, Z_MAX, ALL)                         # n = 0: all-empty views
    assert_planes(empty, RM.render_numpy(p[:0], R, t, Kt, rows, cols, 1, Z_MIN, Z_MAX), "n = 0")
    assert (bits("index", empty["index"]) == RM.EMPTY).all() and (bits("depth", empty["depth"]) == RM.NAN_BITS).all()
    assert not empty["colour"].any() and (bits("normal", empty["normal"]) == RM.NAN_BITS).all()
    for outs in (("depth",), ("index", "normal"), ("colour",)):                                    # a NULL plane is skipped
        got = rd.render(dev, R, t, Kt, rows, cols, 1, Z_MIN, Z_MAX, outs)
        assert tuple(got) == outs
        assert_planes(got, {o: want[o] for o in outs}, str(outs))
    canary = torch.full((2 * rows * cols + 64,), -7.0, dtype=torch.float32, device="cuda")         # nothing is written past the planes
    ctx.wait_torch_stream()
    rd.render_into(dev, R, t, Kt, rows, cols, 1, Z_MIN, Z_MAX, depth=canary)
    ctx.sync()
    assert (canary[2 * rows * cols:] == -7.0).all() and np.array_equal(bits("depth", canary[:2 * rows * cols]).reshape(2, rows, cols), bits("depth", want["depth"]))
    rd.timing(True); st0 = rd.stats(True)
    assert st0 == dict(pairs=0, writes=0, atomics=0)
    still_works()
    ms, st = rd.timing(False), rd.stats(False)
    print("render stage ms:", ms, "splat statistics:", st)
    assert tuple(ms) == RD.STAGES and all(np.isfinite(v) and v >= 0 for v in ms.values()) and sum(ms.values()) > 0
    vis = [RM.visible(p, RM.pose_cw(R[v], t[v]), Kt, rows, cols, 1, Z_MIN, Z_MAX) for v in range(2)]
    writes = sum(int(((np.minimum(pu + 1, cols - 1) - np.maximum(pu - 1, 0) + 1) * (np.minimum(pv + 1, rows - 1) - np.maximum(pv - 1, 0) + 1)).sum())
                 for _, pu, pv, _ in vis)
    assert st["pairs"] == sum(len(v[0]) for v in vis) and st["writes"] == writes and (want["index"] != RM.EMPTY).sum() <= st["atomics"] <= writes
    rd.close()
    for mp, mx in ((0, 10), (10, 0), (1 << 31, 10)):
        with pytest.raises(Exception):
            RD.Renderer(ctx, mp, mx)


# ---- a tracked run ------------------------------------------------------------------------------------------------------------------
def agreement_numpy(index, depth, iD, first, last):
    """rgbid.render.agreement_of restated over the mirror's planes"""
    with np.errstate(divide="ignore", invalid="ignore"):
        own = np.where(np.isfinite(iD) & (iD > 0), F(1) / iD, F(np.nan)).astype(F)
    both = (index != RM.EMPTY) & ((index < first) | (index >= last)) & np.isfinite(own)
    d = np.sort(np.abs(depth[both] - own[both]))
    rank = lambda q: float(d[(q * len(d) + 9) // 10 - 1]) if len(d) else float("nan")
    valid_both = int(((index != RM.EMPTY) & np.isfinite(own)).sum())
    return dict(pixels=int(len(d)), median=rank(5), p90=rank(9)), valid_both


def test_render_on_a_tracked_run(ctx):
    """the 2-chunk noise-free synthetic run of tests/test_gpu_outlier.py at 160 x 120: its novel cloud rendered at three exported
    keyframes' poses equals the mirror; the depth agreement figures equal the same statistic over the mirror's planes.  The figures are
    printed, not asserted (DESIGN.md section 17 holds the measured ones)."""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True)
    kfs = pc.keyframes
    assert len(kfs) >= 3 and len(pc) > 10_000
    sel = [0, len(kfs) // 2, len(kfs) - 1]
    p = pc.numpy()
    R, t = np.stack([kfs[i]["R"] for i in sel]), np.stack([kfs[i]["t"] for i in sel])
    got, want = check(ctx, p, R, t, K_SMALL, rows, cols, 1, 0.05, 20.0, dev=pc.points)
    assert (want["index"] != RM.EMPTY).mean() > 0.2
    figures = RD.depth_agreement(ctx, pc.points, pc.offsets, kfs, K_SMALL, rows, cols, 1)
    assert len(figures) == len(kfs)
    for i, f in enumerate(figures):
        print(f"depth agreement: keyframe {i} at frame {kfs[i]['frame']}: {f['pixels']} pixels, median {f['median']:.6f} m, 90 % {f['p90']:.6f} m")
    run = RD.agreement_summary(figures)
    print(f"depth agreement: {len(kfs)} keyframes, {len(pc)} records, {run['pixels']} pixels, median of medians {run['median']:.6f} m, "
          f"largest 90 % {run['p90']:.6f} m")
    for j, i in enumerate(sel):
        e, valid_both = agreement_numpy(want["index"][j], want["depth"][j], kfs[i]["depthinv"].cpu().numpy(), int(pc.offsets[i]), int(pc.offsets[i + 1]))
        f = figures[i]
        assert f["pixels"] == e["pixels"] <= valid_both
        assert np.array_equal(np.array([f["median"], f["p90"]]), np.array([e["median"], e["p90"]]), equal_nan=True), (i, f, e)


def test_track_dataset_render_options(ctx, tmp_path):
    """--render / --render-check leave the trajectory and the PLY as they were; the PNGs are the in-process rendering of the same run's
    cloud at its keyframes' poses, the printed figures those of depth_agreement"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    views = tmp_path / "views"
    runs = {}
    for name, extra in (("plain", []), ("render", ["--render", str(views), "--render-splat", "2", "--render-check"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--cloud", str(tmp_path / f"{name}.ply")] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = r.stdout
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_render.txt").read_bytes()
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "render.ply").read_bytes()
    assert "render check" not in runs["plain"] and "views of" not in runs["plain"] and "views of" in runs["render"]
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True)
    assert CL.ply_bytes(pc.points) == (tmp_path / "plain.ply").read_bytes()
    kfs = pc.keyframes
    assert sorted(os.listdir(views)) == sorted([f"view_{i:04d}.png" for i in range(len(kfs))] + [f"view_{i:04d}_depth.png" for i in range(len(kfs))])
    want = RD.render_views(ctx, pc.points, np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs]), K_SMALL, rows, cols, 2)
    for i in range(len(kfs)):
        assert np.array_equal(tum.read_png(str(views / f"view_{i:04d}.png")), want["colour"][i].cpu().numpy()), i
        d = tum.read_png(str(views / f"view_{i:04d}_depth.png"))
        assert d.dtype == np.uint16 and np.array_equal(d, RD.depth_png(want["depth"][i])) and (d > 0).any(), i
    figures = RD.depth_agreement(ctx, pc.points, pc.offsets, kfs, K_SMALL, rows, cols, 2)
    said = re.findall(r"render check: keyframe at frame (\d+): (\d+) pixels, median (\S+) m, 90 % (\S+) m", runs["render"])
    assert [(int(a), int(b), c, d) for a, b, c, d in said] == [(k["frame"], f["pixels"], f"{f['median']:.6f}", f"{f['p90']:.6f}") for k, f in zip(kfs, figures)]
    assert f"render check: {len(kfs)} keyframes" in runs["render"]
    # with --optimise the figures come twice, before and after, for the same keyframes
    r = subprocess.run(base + ["--out", str(tmp_path / "traj_opt.txt"), "--cloud", str(tmp_path / "opt.ply"), "--optimise", "--render-check"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    before = re.findall(r"render check before the optimisation: keyframe at frame (\d+): (\d+) pixels", r.stdout)
    after = re.findall(r"render check after the optimisation: keyframe at frame (\d+): (\d+) pixels", r.stdout)
    assert [a for a, _ in before] == [a for a, _ in after] == [str(k["frame"]) for k in kfs]
    assert [(str(k["frame"]), str(f["pixels"])) for k, f in zip(kfs, RD.depth_agreement(ctx, pc.points, pc.offsets, kfs, K_SMALL, rows, cols, 1))] == before
    assert f"render check before the optimisation: {len(kfs)} keyframes" in r.stdout and f"render check after the optimisation: {len(kfs)} keyframes" in r.stdout
    print(r.stdout)
