"""GPU tests of the smoothing stage (include/rgbid_smooth.h, csrc/kernels_smooth.hip, rgbid.smooth): the eight counts, the CSR, the
boundary bytes, the positions after the run and the normals byte for byte against the numpy restatement (tests/smooth_mirror.py) on the
meshes of tests/test_cpu_smooth.py, pinned and not, at 0, 1, 2 and 7 iterations with and without mu, canaries behind every output; either
side of the tiles of the compaction and of the sort; a mesh whose pairs take a second trip of the one-block scan; vertex counts either
side of a change in the sort's pass count; a row of 100 000 neighbours; plans, runs and normals in every order on one handle, exact
capacities; every refusal; and the options of rgbid.tsdf and tools/track_dataset.py.

P is even on every mesh (a pair (v, u) comes with (u, v)), and so is the number of pairs that stay: the sizes "either side" of a tile are the
even ones next to it and the tile itself."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import sequence, smooth as SO, synth, tsdf as TS, tum
from tests import smooth_mirror as SM
from tests import tsdf_mirror as TM
from tests import tsdf_states as S
from tests.test_cpu_smooth import adjacency_of, all_cases, normals_of, smoothed
from tests.test_gpu_cloud import K_SMALL, write_tum_folder
from tests.test_gpu_raycast import loaded
from tests.test_gpu_simplify import chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
CAP_V, CAP_T = 600001, 100001
PAD = 3                                                     # rows behind every output that must keep their canary


def tiles():
    """(RUN_TILE, SORT_TILE) as csrc/voxel_device.h states them"""
    txt = open(os.path.join(ROOT, "rgbid-slam_amd", "csrc", "voxel_device.h")).read()
    num = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, txt).group(1))
    return num("VT") * num("RUN_IPT"), num("VT") * num("SORT_IPT")


RUN_TILE, SORT_TILE = tiles()


@pytest.fixture(scope="module")
def sm(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh of another size"""
    h = SO.Smoother(ctx, CAP_V, CAP_T)
    yield h
    h.close()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def raw(x):
    return x.cpu().numpy().tobytes()


def full(rows, cols, dtype, value):
    return torch.full((rows + PAD,) + cols, value, dtype=dtype, device="cuda")


def assert_planned(sm, tri, adj, normals=True):
    """the plan's counts, and the CSR and the boundary bytes in buffers with PAD canary rows behind them"""
    got = sm.plan(tri, adj["n_v"], normals=normals)
    assert got == adj["counts"], (got, adj["counts"])
    p, n_v = adj["counts"]["pairs"], adj["n_v"]
    off, nb, inc, bd = full(n_v + 1, (), torch.int32, -5), full(p, (), torch.int32, -6), full(p, (), torch.int32, -7), full(n_v, (), torch.uint8, 0xA5)
    sm.ctx.wait_torch_stream()
    sm.adjacency_into(off, nb, inc, bd, p)
    sm.ctx.sync()
    assert raw(off[:n_v + 1]) == adj["offsets"].tobytes() and (off[n_v + 1:] == -5).all()
    assert raw(nb[:p]) == adj["neighbours"].tobytes() and (nb[p:] == -6).all()
    assert raw(inc[:p]) == adj["incidences"].tobytes() and (inc[p:] == -7).all()
    assert raw(bd[:n_v]) == adj["boundary"].tobytes() and (bd[n_v:] == 0xA5).all()


def assert_run(sm, vdev, exp, iterations, lam=0.5, mu=-0.53, pin=False):
    """one run into a buffer with PAD canary rows: the positions' bytes, the canary, the input untouched"""
    n_v = len(exp)
    before = raw(vdev)
    out = full(n_v, (3,), torch.float32, 7.0)
    sm.ctx.wait_torch_stream()
    sm.run_into(vdev, out[:n_v], iterations, lam, mu, pin)
    sm.ctx.sync()
    got = out[:n_v].cpu().numpy()
    assert got.tobytes() == exp.tobytes(), (iterations, lam, mu, pin, np.nonzero((got.view(U32) != exp.view(U32)).any(1))[0][:10])
    assert (out[n_v:] == 7.0).all() and raw(vdev) == before


def assert_normals(sm, vdev, exp):
    n_v = len(exp)
    out = full(n_v, (3,), torch.float32, -3.0)
    sm.ctx.wait_torch_stream()
    sm.normals_into(vdev, out[:n_v])
    sm.ctx.sync()
    assert raw(out[:n_v]) == exp.tobytes() and (out[n_v:] == -3.0).all()


def assert_smoothed(sm, m, iterations=(0, 1, 2), pins=(False, True), mus=(-0.53, 0.0)):
    """a mesh that is no case of the CPU file: plan, runs and normals against the mirror -> the adjacency"""
    v = np.ascontiguousarray(m["vertices"], F)
    adj = SM.adjacency(m["triangles"], len(v))
    vdev = dev(v)
    assert_planned(sm, dev(m["triangles"]), adj)
    for pin in pins:
        for mu in mus:
            for n in iterations:
                assert_run(sm, vdev, SM.smooth(v, None, n, 0.5, mu, pin, adj=adj), n, 0.5, mu, pin)
    assert_normals(sm, vdev, SM.normals(v, adj))
    return adj


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_cases_against_the_mirror(sm, name):
    """0, 1, 2 and 7 iterations with and without mu are 0, 1, 2, 4, 7 and 14 passes: both parities of the ping-pong"""
    m, adj = all_cases()[name], adjacency_of(name)
    tri, vdev = dev(m["triangles"]), dev(m["vertices"])
    assert_planned(sm, tri, adj)
    for pin in (False, True):
        for mu in (-0.53, 0.0):
            for n in (0, 1, 2, 7):
                assert_run(sm, vdev, smoothed(name, n, 0.5, mu, pin), n, 0.5, mu, pin)
    assert_normals(sm, vdev, normals_of(name))
    after = smoothed(name, 7)
    assert_normals(sm, dev(after), SM.normals(after, adj))
    out = sm.run(vdev, 2, pin_boundary=True)                   # the allocating forms
    assert raw(out) == smoothed(name, 2, 0.5, -0.53, True).tobytes() and raw(sm.normals(vdev)) == normals_of(name).tobytes()
    got = sm.adjacency()
    assert raw(got["offsets"]) == adj["offsets"].tobytes() and raw(got["neighbours"]) == adj["neighbours"].tobytes()
    assert raw(got["incidences"]) == adj["incidences"].tobytes() and raw(got["boundary"]) == adj["boundary"].tobytes()


def test_a_vertex_that_overflows_stays(sm):
    """the hand-built mesh under lambda = 1e-9, mu = -1: vertex 22 becomes inf in the first mu pass, then stays and is skipped"""
    m, adj = all_cases()["hand"], adjacency_of("hand")
    assert_planned(sm, dev(m["triangles"]), adj)
    exp = smoothed("hand", 2, 1e-9, -1.0)
    assert exp[22, 0] == np.inf
    assert_run(sm, dev(m["vertices"]), exp, 2, 1e-9, -1.0)
    assert_run(sm, dev(m["vertices"]), smoothed("hand", 3, 1.0, -2.0, True), 3, 1.0, -2.0, True)      # the ends of both ranges


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
def strip_mesh(k, n_v, singles=0, degenerate=0, duplicates=0, seed=0):
    """a strip of k triangles over the first k + 2 vertices (4 k + 2 rows), `singles` separate triangles behind it (6 rows each),
    `degenerate` triangles (a, a, b) over strip vertices (2 dropped pairs each, no new row) and `duplicates` repeats of strip triangles (no
    new row), shuffled, over n_v vertices at random positions"""
    rng = np.random.default_rng(seed)
    strip = np.arange(k)[:, None] + np.arange(3)[None, :]
    single = k + 2 + 3 * np.arange(singles)[:, None] + np.arange(3)[None, :]
    a = rng.integers(0, k, degenerate)
    tri = np.concatenate([strip, single, np.stack([a, a, a + 1], 1), strip[rng.integers(0, k, duplicates)]]).astype(U32)
    assert tri.max() < n_v
    return dict(vertices=rng.uniform(-1, 1, (n_v, 3)).astype(F), triangles=tri[rng.permutation(len(tri))])


@pytest.mark.parametrize("n_v", [2047, 2048, 2049])
def test_vertex_counts_either_side_of_a_tile(sm, n_v):
    adj = assert_smoothed(sm, strip_mesh(n_v - 2, n_v, seed=n_v), iterations=(2,))
    assert adj["counts"]["isolated"] == 0 and adj["counts"]["pairs"] == 4 * (n_v - 2) + 2


@pytest.mark.parametrize("k, singles", [(511, 0), (510, 1), (512, 0), (1023, 0), (1022, 1), (1024, 0)])
def test_rows_either_side_of_a_tile(sm, k, singles):
    """P = 2046, 2048, 2050 and 4094, 4096, 4098, with duplicates and degenerate triangles that add pairs and no row"""
    m = strip_mesh(k, k + 2 + 3 * singles + 5, singles, degenerate=7, duplicates=40, seed=k)
    adj = assert_smoothed(sm, m, iterations=(2,))
    assert adj["counts"]["pairs"] == 4 * k + 2 + 6 * singles and adj["counts"]["pairs"] in (2046, 2048, 2050, 4094, 4096, 4098)
    assert adj["counts"]["dropped"] == 14 and adj["counts"]["isolated"] == 5 and adj["counts"]["non_manifold"] > 0


@pytest.mark.parametrize("n_t", [341, 342, 682, 683, 1365, 1366])
def test_triangle_counts_either_side_of_a_tile(sm, n_t):
    """6 n_t = 2046 | 2052, 4092 | 4098 and 3 n_t = 2046 | 2049, 4095 | 4098; with two (a, a, b) among 342 and 683 triangles the pairs
    that stay are exactly 2048 and 4094"""
    m = strip_mesh(n_t - 2, n_t + 10, degenerate=2, seed=n_t)
    adj = assert_smoothed(sm, m, iterations=(1,))
    assert int(adj["incidences"].sum()) == 6 * n_t - 4 and len(adj["corners"]) == 3 * n_t
    rng = np.random.default_rng(n_t)
    assert_smoothed(sm, dict(vertices=rng.random((500, 3)), triangles=rng.integers(0, 500, (n_t, 3)).astype(U32)), iterations=(1,))


def test_pairs_take_a_second_scan_trip(sm):
    """100 000 triangles are 600 000 pairs, 293 tiles of the compaction: more than the 256 the one-block scan takes in one trip; over
    600 000 vertices most of which no triangle names"""
    rng = np.random.default_rng(1)
    tri = rng.integers(0, 600000, (100000, 3)).astype(U32)
    tri[::50] = rng.integers(0, 40, (2000, 3))                  # duplicates, non-manifold edges and degenerate triangles among the first vertices
    tri[-1] = (599999, 0, 599998)
    m = dict(vertices=rng.uniform(-1, 1, (600000, 3)).astype(F), triangles=tri)
    m["vertices"][5::1000, 1] = np.nan
    adj = assert_smoothed(sm, m, iterations=(2,), pins=(False,), mus=(-0.53,))
    c = adj["counts"]
    assert c["isolated"] > 300000 and c["pairs"] > 256 * RUN_TILE and c["dropped"] > 0 and c["non_manifold"] > 0
    assert (600000 - c["dropped"] + RUN_TILE - 1) // RUN_TILE > 256


@pytest.mark.parametrize("n_v", [255, 256, 257, 65535, 65536, 65537])
def test_vertex_counts_either_side_of_a_sort_pass(sm, n_v):
    """the sentinel n_v of the sorts has 8, 9, 16 and 17 bits: one, two and three passes per round"""
    rng = np.random.default_rng(n_v)
    tri = rng.integers(0, n_v, (6000, 3)).astype(U32)
    tri[:3000] = rng.integers(n_v - 40, n_v, (3000, 3))          # the largest indices
    tri[-1] = (n_v - 1, 0, n_v - 2)
    adj = assert_smoothed(sm, dict(vertices=rng.random((n_v, 3)), triangles=tri), iterations=(1,), pins=(False,))
    assert int(adj["neighbours"].max()) == n_v - 1 and adj["counts"]["dropped"] > 100 and adj["counts"]["non_manifold"] > 100


def test_a_row_of_100000_neighbours(sm):
    """the ordered double sum, the gather of four and its tail over one row; the values lose bits in any other order of adding"""
    n = 100000
    rng = np.random.default_rng(3)
    v = (rng.random((n + 2, 3)) * np.array([1.0, 1e-3, 1e3])).astype(F)
    v[7], v[8], v[9] = (1, 1, 1), (1e30, 3e38, 1), (-1e30, -3e38, 1)
    tri = np.stack([np.full(n, n + 1), np.arange(n), np.arange(1, n + 1)], 1).astype(U32)
    adj = assert_smoothed(sm, dict(vertices=v, triangles=tri), iterations=(1, 2), pins=(False,))
    assert adj["counts"]["max_degree"] == n + 1
    single = v[:n + 1].sum(0, dtype=F) / F(n + 1)               # float32 sums round in every add: the mean has other bits
    hub = SM.smooth_pass(v, adj, 1.0)[n + 1]
    assert single.tobytes() != hub.tobytes()


# ---- life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_plans_and_runs_on_one_handle(ctx):
    """a handle of exactly the largest mesh's sizes: a smaller mesh after a larger one and back, no vertices in between; two runs and a
    normals call on one plan; a plan without the normals flag; the adjacency into exactly P rows and into one row fewer"""
    cases = all_cases()
    names = ("random", "hand", "no_vertices", "random", "sphere", "no_triangles", "hand", "open_sphere", "random")
    cap_v, cap_t = (max(len(cases[n][k]) for n in names) for k in ("vertices", "triangles"))
    h = SO.Smoother(ctx, cap_v, cap_t)
    try:
        for name in names:
            m, adj = cases[name], adjacency_of(name)
            tri, vdev = dev(m["triangles"]), dev(m["vertices"])
            assert_planned(h, tri, adj)
            assert_run(h, vdev, smoothed(name, 2), 2)
            assert_normals(h, vdev, normals_of(name))
            assert_run(h, vdev, smoothed(name, 1, 0.5, 0.0, True), 1, 0.5, 0.0, True)
        assert_planned(h, tri, adj, normals=False)               # the same mesh without the corner table
        out = torch.full((cap_v, 3), -3.0, dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError):
            h.normals(vdev)
        with pytest.raises(Exception, match="rgbid error -1"):
            h.normals_into(vdev, out)
        ctx.sync()
        assert (out == -3.0).all()
        assert_run(h, vdev, smoothed("random", 7), 7)
        p = adj["counts"]["pairs"]
        nb, inc = torch.full((p,), -6, dtype=torch.int32, device="cuda"), torch.full((p,), -7, dtype=torch.int32, device="cuda")
        ctx.wait_torch_stream()
        with pytest.raises(Exception, match="rgbid error -1"):
            h.adjacency_into(None, nb[:p - 1], inc, None, p - 1)
        ctx.sync()
        assert (nb == -6).all() and (inc == -7).all()
        h.adjacency_into(None, nb, inc, None, p)
        ctx.sync()
        assert raw(nb) == adj["neighbours"].tobytes() and raw(inc) == adj["incidences"].tobytes()
        with pytest.raises(ValueError):
            h.plan(tri, cap_v + 1)                               # above the capacity
        h.timing(True)
        assert_planned(h, tri, adj)
        assert_run(h, vdev, smoothed("random", 2), 2)
        assert_normals(h, vdev, normals_of("random"))
        ms = h.timing(False)
        print("smooth stage ms:", ms)
        assert tuple(ms) == SO.STAGES and all(np.isfinite(x) and x > 0 for x in ms.values())
    finally:
        h.close()


def test_refusals_and_reuse(sm):
    L = sm.L
    m, adj = all_cases()["sphere"], adjacency_of("sphere")
    tri, vdev = dev(m["triangles"]), dev(m["vertices"])
    n_v, n_t = len(m["vertices"]), len(m["triangles"])
    counts = (C.c_ulonglong * 8)()

    def still_works():
        assert_planned(sm, tri, adj)
        assert_run(sm, vdev, smoothed("sphere", 2), 2)
        assert_normals(sm, vdev, normals_of("sphere"))

    out = torch.zeros((n_v + 1, 3), dtype=torch.float32, device="cuda")
    buf = torch.zeros(adj["counts"]["pairs"] + n_v + 2, dtype=torch.int32, device="cuda")
    pv, pt, po, pb = vdev.data_ptr(), tri.data_ptr(), out.data_ptr(), buf.data_ptr()
    plan = lambda nv=n_v, nt=n_t, t=pt, flags=1: L.rgbid_smooth_plan(sm._h, nv, nt, t, flags, counts)
    run = lambda i=pv, o=po, n=2, lam=0.5, mu=-0.53, flags=0: L.rgbid_smooth_run(sm._h, i, o, n, lam, mu, flags)
    adjacency = lambda off=pb, nb=None, inc=None, bd=None, cap=adj["counts"]["pairs"]: L.rgbid_smooth_adjacency(sm._h, off, nb, inc, bd, cap)
    still_works()
    # a triangle that names a vertex that does not exist: the plan is refused, the former one is gone, the next one is right
    for where in (0, n_t // 2, n_t - 1):
        for value in (n_v, 0xFFFFFFFF):
            bad = np.array(m["triangles"], U32)
            bad[where, where % 3] = value
            with pytest.raises(Exception, match="rgbid error -1"):
                sm.plan(dev(bad), n_v, normals=True)
            assert run() == -1 and adjacency() == -1 and L.rgbid_smooth_normals(sm._h, pv, po) == -1
        still_works()
    # the host-side refusals keep the plan: the calls after them are the former plan's
    for r in (lambda: plan(nv=CAP_V + 1), lambda: plan(nt=CAP_T + 1), lambda: plan(t=None), lambda: plan(t=pt + 1), lambda: plan(t=pt + 2),
              lambda: plan(nv=0), lambda: plan(flags=2), lambda: plan(flags=0x80000001)):
        sm.ctx.wait_torch_stream()
        assert r() == -1
        assert_run(sm, vdev, smoothed("sphere", 1), 1)
        assert_normals(sm, vdev, normals_of("sphere"))
    inf, nan = float("inf"), float("nan")
    for r in (lambda: run(i=None), lambda: run(o=None), lambda: run(i=pv + 2), lambda: run(o=po + 1), lambda: run(o=pv), lambda: run(i=po),
              lambda: run(i=po + 12), lambda: run(n=4097),     # in == out, and in one row inside out
              lambda: run(n=0xFFFFFFFF), lambda: run(lam=0.0), lambda: run(lam=-0.5), lambda: run(lam=1.5), lambda: run(lam=nan), lambda: run(lam=inf),
              lambda: run(mu=0.1), lambda: run(mu=-2.5), lambda: run(mu=nan), lambda: run(mu=-inf), lambda: run(flags=2), lambda: run(flags=0x80000001),
              lambda: adjacency(cap=adj["counts"]["pairs"] - 1), lambda: adjacency(off=pb + 2), lambda: adjacency(nb=pb + 1), lambda: adjacency(inc=pb + 3),
              lambda: L.rgbid_smooth_normals(sm._h, None, po), lambda: L.rgbid_smooth_normals(sm._h, pv, None),
              lambda: L.rgbid_smooth_normals(sm._h, pv + 2, po), lambda: L.rgbid_smooth_normals(sm._h, pv, po + 2)):
        assert r() == -1
    sm.ctx.sync()
    assert not out.any() and not buf.any() and raw(vdev) == m["vertices"].tobytes()
    assert run() == 0 and adjacency() == 0
    sm.ctx.sync()
    assert raw(out[:n_v]) == smoothed("sphere", 2).tobytes() and not out[n_v:].any()
    assert raw(buf[:n_v + 1]) == adj["offsets"].tobytes() and not buf[n_v + 1:].any()
    still_works()
    for bad in (dict(iterations=-1), dict(iterations=4097), dict(iterations=1, lam=0), dict(iterations=1, mu=1)):
        with pytest.raises(ValueError):                     # the Python checks come first
            sm.run(vdev, **bad)
    with pytest.raises(ValueError):
        sm.run(vdev[:-1], 1)
    with pytest.raises(ValueError):
        sm.normals(tri)
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        with pytest.raises(Exception):
            SO.Smoother(sm.ctx, v, t)
    still_works()


# ---- through the volume, a tracked run and the command line -----------------------------------------------------------------------------
def mirrored_smooth(v, t, normals=True, **kw):
    """the one-shot's result from the mirrors: positions, normals of the smoothed surface, the figures"""
    kw = TS.smooth_arg(kw)
    adj = SM.adjacency(t, len(v))
    out = SM.smooth(v, None, kw["iterations"], kw["lam"], kw["mu"], kw["pin_boundary"], adj=adj)
    info = dict(adj["counts"], vertices=len(v), triangles=len(t), **kw)
    return out, SM.normals(out, adj) if normals else None, info


def test_volume_extract_smooths(ctx):
    """a large and a small sphere in 128 x 64 x 64 voxels through Volume.extract(min_component=..., simplify=..., smooth=..., normals=True)
    against extract, then the mirrors: fragments first, then decimation, then smoothing with the normals of the smoothed surface"""
    m = TM.Volume(128, 64, 64, (0.0, 0.0, 0.0), 0.05, 0.2)
    big, W = TM.sphere_state(m, (3.2, 1.6, 1.6), 1.5)
    small, _ = TM.sphere_state(m, (0.4, 0.4, 0.4), 0.25)
    vol = TS.Volume(ctx, m.n, 1, colour=False)
    vol.configure(128, 64, 64, [0.0, 0.0, 0.0], 0.05, 0.2)
    vol.set_state(torch.from_numpy(np.minimum(big, small)).cuda(), torch.from_numpy(W.view(np.int32)).cuda())
    host = [x.cpu().numpy() for x in vol.extract(1, normals=True)]
    host[2] = host[2].view(U32)
    exp, info, _ = chain(*host, 0.2, min_triangles=5000)
    ev, en, figures = mirrored_smooth(exp["vertices"], exp["triangles"], iterations=5, pin_boundary=True)
    v, c, t, n = vol.extract(1, normals=True, min_component=5000, simplify=0.2, smooth=dict(iterations=5, pin_boundary=True))
    assert raw(v) == ev.tobytes() and raw(n) == en.tobytes() and raw(t) == exp["triangles"].tobytes()
    assert (c is None and exp["colours"] is None) or raw(c) == exp["colours"].tobytes()
    assert vol.last_smooth == figures and vol.last_simplify == info, (vol.last_smooth, figures)
    assert raw(v) != exp["vertices"].tobytes() and raw(n) != exp["normals"].tobytes()
    # smoothing alone, without normals and without colours
    ev, _, figures = mirrored_smooth(host[0], host[2], normals=False, iterations=3)
    fv, fc, ft = vol.extract(1, colours=False, smooth=3)
    assert fc is None and raw(fv) == ev.tobytes() and raw(ft) == host[2].tobytes() and vol.last_smooth == figures
    vol.close()


def test_fuse_smooths_a_tracked_run(ctx):
    """the tracked run of tests/test_gpu_tsdf.py through fuse(smooth=10) against fuse, then the mirror.  The figures are printed and
    asserted against the mirror only (DESIGN.md section 24 holds the measured ones)."""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                         keyframe_colour=True)
    v, c, t, nrm, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, normals=True)
    assert "smooth" not in info
    sv, sc, st, sn, sinfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, normals=True, smooth=10)
    ev, en, figures = mirrored_smooth(v.cpu().numpy(), t.cpu().numpy().view(U32), iterations=10)
    print("tracked run:", sinfo["smooth"])
    assert sinfo["smooth"] == figures and {k: sinfo[k] for k in info} == info
    assert raw(sv) == ev.tobytes() and raw(sn) == en.tobytes() and raw(st) == raw(t) and raw(sc) == raw(c)
    assert raw(sv) != raw(v)


def test_poisoned_state_keeps_its_nan_vertices(ctx):
    """the extraction writes NaN vertices on a poisoned state: they pass through as bytes, their neighbours skip
    them and their triangles give no normal"""
    mirror = S.poisoned_state()
    vol = loaded(ctx, mirror)
    host = [x.cpu().numpy() for x in vol.extract(1, normals=True)]
    host[2] = host[2].view(U32)
    bad = ~np.isfinite(host[0]).all(1)
    assert bad.sum() >= 100
    ev, en, figures = mirrored_smooth(host[0], host[2], iterations=3)
    v, c, t, n = vol.extract(1, normals=True, smooth=3)
    assert raw(v) == ev.tobytes() and raw(n) == en.tobytes() and vol.last_smooth == figures
    assert ev[bad].tobytes() == host[0][bad].tobytes() and np.isfinite(ev[~bad]).all() and np.isfinite(en).all()
    vol.close()


def test_track_dataset_mesh_smooth_option(ctx, tmp_path):
    """without the new option the PLY and the trajectory are what fuse gives today; with --mesh-smooth the file holds exactly fuse's
    smoothed tensors, the trajectory and the mesh line are unchanged and one more line tells what the smoothing did"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("smoothed", ["--mesh-normals", "--mesh-smooth", "5", "--mesh-smooth-mu", "-0.5", "--mesh-smooth-pin-boundary"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply"), "--mesh-voxel", "0.05",
                                   "--mesh-min-weight", "2"] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = r.stdout
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True, keyframe_colour=True)
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_smoothed.txt").read_bytes()
    v, c, t, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True)
    sv, sc, st, sn, sinfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True, normals=True,
                                    smooth=dict(iterations=5, mu=-0.5, pin_boundary=True))
    assert (tmp_path / "plain.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0
    assert (tmp_path / "smoothed.ply").read_bytes() == TS.mesh_ply_bytes(sv, sc, st, sn) and raw(st) == raw(t) and raw(sv) != raw(v)
    line = f"{info['voxels']} voxels of 0.05 m (truncation 0.2 m), {info['touched']} touched, {v.shape[0]} vertices, {t.shape[0]} triangles"
    assert line in said["plain"] and line in said["smoothed"] and "mesh smooth" not in said["plain"]
    f = sinfo["smooth"]
    assert (f"mesh smooth: 5 iterations of lambda 0.5, mu -0.5, {f['edges']} edges, {f['boundary_vertices']} boundary vertices, pinned") in said["smoothed"], \
        said["smoothed"]
    mesh_lines = lambda s: [l.replace("smoothed.ply", "plain.ply") for l in s.splitlines() if " mesh of " in l]
    assert mesh_lines(said["plain"]) == mesh_lines(said["smoothed"]) and len(mesh_lines(said["plain"])) == 1
