"""GPU tests of the colour alignment (include/rgbid_colouralign.h, csrc/kernels_colouralign.hip, rgbid.colouralign): the result records
and the targets S, W, used byte for byte against the numpy restatement (tests/colouralign_mirror.py), a canary element behind every
output; the wave, block and upper-tree edges of the lattice at 1, 2 and 17 views under three schedules and two strides; every
combination of optional inputs; the five statuses; waves without a used pair beside used ones; the Huber threshold met exactly; repeated
calls and a handle of exact capacity; every host-side refusal; the stage timer; the box filter; refine_keyframes against the mirror fed
the device rasteriser's planes; rgbid.tsdf.fuse and tools/track_dataset.py with and without the option."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import colouralign as CA, raster as RS, recolour as RC, synth, tsdf as TS
from rgbid.render import Pose
from tests import colouralign_mirror as CM
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U8 = np.float32, np.uint8
CAP_N, CAP_V = 4097, 17
ROWS, COLS = 48, 64
K = (70.0, 69.0, 31.5, 23.5)
PRM = dict(z_min=0.5, z_max=4.0, surface_tolerance=0.05, measured_tolerance=0.05, min_cos=0.2, two_sided=False)
SCHEDULES = ((1, 1), (2, 2), (3, 1))
OPTIONAL = ("normals", "surface", "depthinv")


@pytest.fixture(scope="module")
def ca(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh of another size and other views"""
    h = CA.ColourAligner(ctx, CAP_N, CAP_V)
    yield h
    h.close()


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def wavy(x, y):
    """the surface of the cases, 1.5 m in front of the cameras, its waves well below the surface tolerance"""
    return 1.5 + 0.01 * np.sin(2.0 * x) * np.cos(1.5 * y)


@pytest.fixture(scope="module")
def views17():
    """17 views of the textured plane z = 1.5: poses near the identity, smooth colour images (three different channels), the plane's
    depth with holes, its inverse depth with holes; computed once"""
    r = np.random.default_rng(11)
    u, v = np.meshgrid(np.arange(COLS, dtype=np.float64), np.arange(ROWS, dtype=np.float64))
    out = dict(R=[], t=[], colours=[], surface=[], depthinv=[])
    for k in range(17):
        R, t = CM.perturb(np.eye(3), np.zeros(3), 0.01 * (k > 0), 100 + k)
        # the image: the texture at the point where the pixel's ray meets z = 1.5
        d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1) @ R.T
        lam = (1.5 - t[2]) / d[..., 2]
        x, y = t[0] + lam * d[..., 0], t[1] + lam * d[..., 1]
        g = CM.texture(3.0 * x, 3.0 * y)
        img = np.stack([np.clip(g + 20 * np.sin(5 * x + c), 0, 255) for c in range(3)], -1)
        out["R"].append(R); out["t"].append(t)
        out["colours"].append(np.floor(img + 0.5).astype(U8))
        z = (lam * (d @ R)[..., 2]).astype(F)                       # the depth of that point along the camera's axis
        out["surface"].append(np.where(r.random((ROWS, COLS)) < 0.02, np.nan, z).astype(F))
        out["depthinv"].append(np.where(r.random((ROWS, COLS)) < 0.02, 0.0, 1.0 / z).astype(F))
    return {k: np.stack(x) for k, x in out.items()}


def mesh_points(n, seed=2):
    """n vertices of the surface in raster order (so that 64 consecutive ones are neighbours), some outside every image, one not finite;
    normals towards the cameras, some zero"""
    r = np.random.default_rng(seed)
    nx = max(int(np.ceil(np.sqrt(n * 4 / 3))), 1)
    i = np.arange(n)
    x, y = (i % nx) / max(nx - 1, 1) * 1.5 - 0.75, (i // nx) / max((n - 1) // nx, 1) * 1.1 - 0.55
    pos = np.stack([x, y, wavy(x, y)], 1).astype(F)
    nrm = np.stack([0.3 * r.normal(size=n), 0.3 * r.normal(size=n), -np.ones(n)], 1).astype(F)
    if n > 5:
        pos[5] = np.nan
        nrm[::9] = 0
    return pos, nrm


def case(views, n, V, drop=()):
    pos, nrm = mesh_points(n)
    c = dict(vertices=pos, normals=nrm, R=views["R"][:V], t=views["t"][:V], colours=views["colours"][:V], surface=views["surface"][:V],
             depthinv=views["depthinv"][:V])
    for k in drop:
        c[k] = None
    return c


def run_device(ca, c, fixed=(0,), rows=ROWS, cols=COLS, K_=K, prm=PRM, **rule):
    """one run into outputs with a canary element behind them -> (records, S, W, used) as numpy, the canaries checked"""
    V, n = len(c["R"]), len(c["vertices"])
    n_l = (n + rule.get("stride", 1) - 1) // rule.get("stride", 1)
    result = torch.full(((V + 1) * 560,), 0xA5, dtype=torch.uint8, device="cuda")
    S, W = (torch.full((n_l + 1,), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    used = torch.full((n_l + 1,), -9, dtype=torch.int32, device="cuda")
    t = {k: dev(c[k]) for k in ("vertices", "normals", "colours", "surface", "depthinv")}
    ca.ctx.wait_torch_stream()
    ca.run_into(result[:V * 560], t["vertices"], c["R"], c["t"], K_, rows, cols, t["colours"], surface=t["surface"], depthinv=t["depthinv"],
                normals=t["normals"], fixed=fixed, **prm, **rule)
    ca.targets_into(S[:n_l], W[:n_l], used[:n_l])
    ca.ctx.sync()
    assert (result[V * 560:] == 0xA5).all() and int(S[n_l]) == -7 and int(W[n_l]) == -7 and int(used[n_l]) == -9
    return (result[:V * 560].cpu().numpy().view(CA.RESULT), S[:n_l].cpu().numpy().view(np.uint64), W[:n_l].cpu().numpy().view(np.uint64),
            used[:n_l].cpu().numpy().view(np.uint32))


def run_mirror(c, fixed=(0,), rows=ROWS, cols=COLS, K_=K, prm=PRM, trace=None, **rule):
    return CM.run(c["vertices"], c["R"], c["t"], K_, rows, cols, c["colours"], surface=c["surface"], depthinv=c["depthinv"], normals=c["normals"],
                  fixed=fixed, params=prm, trace=trace, **rule)


def assert_same(got, exp, what=""):
    rec, S, W, used = got
    for f in ("status", "iterations", "used", "pose", "sums"):
        assert rec[f].tobytes() == exp["records"][f].tobytes(), (what, f, rec[f], exp["records"][f])
    assert rec.tobytes() == exp["records"].tobytes(), what
    assert S.tobytes() == exp["S"].tobytes() and W.tobytes() == exp["W"].tobytes() and used.tobytes() == exp["used"].tobytes(), what


@pytest.mark.parametrize("V", [1, 2, 17])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_wave_block_and_tree_edges(ca, views17, n, V):
    """4 097 vertices are 65 groups of 64: two rounds of the upper tree.  A single view is not held: it finds no target, so its system of
    zero used pairs and its solve run at every size and end FEW"""
    c = case(views17, n, V)
    seen = set()
    for (rounds, iterations), stride in itertools.product(SCHEDULES, (1, 3)):
        rule = dict(rounds=rounds, iterations=iterations, stride=stride, huber=12.0, eps=1e-9)
        exp = run_mirror(c, fixed=() if V == 1 else (0,), **rule)
        assert_same(run_device(ca, c, fixed=None if V == 1 else (0,), **rule), exp, (n, V, rule))
        seen |= set(exp["records"]["status"].tolist())
    if V == 17 and n >= 255:
        assert CM.RUNNING in seen and CM.FIXED in seen
    if V == 1:
        assert seen == {CM.FEW} and exp["records"]["iterations"].tolist() == [1]
    elif n == 0:
        assert seen == {CM.FIXED, CM.FEW}


@pytest.mark.parametrize("n,V", [(257, 17), (4097, 17), (4097, 16), (65, 2), (0, 17)])
def test_both_forms_of_the_target_pass(ca, views17, n, V):
    """all views per vertex, and chunks of 16 views over blocks with integer atomics: the same bytes, also where the second chunk holds one
    view, where there is one chunk and where the lattice is empty; the library's own choice is one of them"""
    c = case(views17, n, V)
    rule = dict(rounds=2, iterations=1, stride=1)
    exp = run_mirror(c, **rule)
    assert n == 0 or (exp["used"] > 1).any()
    try:
        for form in ("walk", "chunks", "auto"):
            ca.target_form(form)
            assert_same(run_device(ca, c, **rule), exp, form)
            # a larger lattice before it leaves sums behind that the chunks must not add to
            assert_same(run_device(ca, case(views17, max(n // 3, 1), V), **rule), run_mirror(case(views17, max(n // 3, 1), V), **rule), form)
            assert_same(run_device(ca, c, **rule), exp, form)
    finally:
        ca.target_form("auto")
    with pytest.raises(ValueError):
        ca.target_form("atomics")
    assert ca.L.rgbid_colouralign_set_target_form(ca._h, 3) == -1 and ca.L.rgbid_colouralign_set_target_form(ca._h, -1) == -1


@pytest.mark.parametrize("drop", [d for k in range(4) for d in itertools.combinations(OPTIONAL, k)])
def test_every_combination_of_inputs(ca, views17, drop):
    c = case(views17, 257, 3, drop)
    for stride in (1, 3):
        rule = dict(rounds=2, iterations=2, stride=stride)
        exp = run_mirror(c, **rule)
        assert_same(run_device(ca, c, **rule), exp, (drop, stride))
        assert (exp["records"]["used"][1:, 0] > 6).all()


def test_the_five_statuses_in_one_call(ca, views17):
    """view 0 is held (FIXED), view 1 shows a constant image (SINGULAR), view 2 looks away (FEW), view 3 starts at a true pose and
    meets eps = 0.02 (CONVERGED), view 4 starts 0.01 off, is drawn by the constant image's share of the targets and does not in two
    iterations (RUNNING); and a single view finds no target (FEW)"""
    c = case(views17, 600, 5)
    c["colours"] = c["colours"].copy(); c["R"] = c["R"].copy(); c["t"] = c["t"].copy()
    c["colours"][1] = 99
    c["R"][2] = np.diag([1.0, -1.0, -1.0])
    c["R"][3], c["t"][3] = c["R"][0], c["t"][0]
    c["colours"][3], c["surface"], c["depthinv"] = c["colours"][0], None, None
    rule = dict(rounds=1, iterations=2, eps=2e-2)
    exp = run_mirror(c, **rule)
    assert exp["records"]["status"].tolist() == [CM.FIXED, CM.SINGULAR, CM.FEW, CM.CONVERGED, CM.RUNNING], exp["records"]["status"]
    assert_same(run_device(ca, c, **rule), exp)
    for eps, status in ((1.0, CM.CONVERGED), (1e-12, CM.RUNNING)):
        rule = dict(rounds=2, iterations=2, eps=eps)
        exp = run_mirror(c, **rule)
        assert exp["records"]["status"][4] == status
        assert_same(run_device(ca, c, **rule), exp)
    one = {k: (None if x is None else x[4:5] if k not in ("vertices", "normals") else x) for k, x in c.items()}
    exp = run_mirror(one, fixed=(), **rule)
    assert exp["records"]["status"].tolist() == [CM.FEW] and exp["records"]["iterations"].tolist() == [1]
    assert_same(run_device(ca, one, fixed=None, **rule), exp)


def test_waves_without_a_used_pair_beside_used_ones(ca, views17):
    """a strip of 64 x 48 vertices in column order, each column one group of 64; every view sees under a quarter of it, views 0 and 1 the
    same part, views 2 and 3 another: most waves of a running view's system hold no used pair and store +0.0 without the tree"""
    ys, xs = np.meshgrid(np.linspace(-0.4, 0.4, 64), np.linspace(-6.0, 6.0, 48))
    pos = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(xs.size, 1.5)], 1).astype(F)
    c = dict(vertices=pos, normals=None, surface=None, depthinv=None)
    c["R"] = views17["R"][:4].copy(); c["t"] = views17["t"][:4].copy()
    c["t"][2:, 0] += 4.0
    c["colours"] = views17["colours"][:4]
    trace = []
    rule = dict(rounds=2, iterations=2)
    exp = run_mirror(c, fixed=(0,), trace=trace, **rule)
    assert len(trace) == 12
    for _, _, v, per_group in trace:
        assert len(per_group) == 48 and 0 < (per_group > 0).sum() < 12 and (per_group == 0).sum() > 36, (v, per_group)
    assert (exp["records"]["used"][1:, 0] > 6).all()
    assert_same(run_device(ca, c, **rule), exp)


def test_huber_met_exactly_and_one_ulp_either_side(ca):
    """eight vertices on the optical axis; view 0 (held) shows the edge between grey 0 and 90 there (g = 45), view 1 a constant 5:
    C = 25 and f = -20 for view 1.  wh = 1 at huber = 20 and one ulp above, huber / 20 one ulp below"""
    pos = np.tile(np.array([[0.0, 0.0, 1.0]], F), (8, 1))
    K_ = (50.0, 50.0, 7.5, 7.5)
    img = np.zeros((2, 16, 16, 3), U8); img[0, :, 8:] = 90; img[1] = 5
    c = dict(vertices=pos, normals=None, surface=None, depthinv=None, R=np.stack([np.eye(3)] * 2), t=np.zeros((2, 3)), colours=img)
    for huber, unit in ((20.0, True), (float(np.nextafter(F(20), F(30))), True), (float(np.nextafter(F(20), F(0))), False)):
        rule = dict(rounds=1, iterations=1, huber=huber)
        exp = run_mirror(c, rows=16, cols=16, K_=K_, **rule)
        e = exp["records"]["sums"][1, 0, 27]
        assert exp["records"]["used"][1, 0] == 8 and (e == 8 * 400.0) == unit and e == 8 * ((1.0 if unit else float(np.float64(F(huber)) / 20.0)) * -20.0) * -20.0
        assert_same(run_device(ca, c, rows=16, cols=16, K_=K_, **rule), exp, huber)


def test_repeated_calls_and_a_handle_of_exact_capacity(ctx, views17):
    c1, c2 = case(views17, 300, 4), case(views17, 129, 2, drop=("normals",))
    c2 = dict(c2, colours=c2["colours"][:, :40, :50].copy(), surface=c2["surface"][:, :40, :50].copy(), depthinv=c2["depthinv"][:, :40, :50].copy())
    h = CA.ColourAligner(ctx, 300, 4)
    try:
        rule = dict(rounds=2, iterations=1)
        e1, e2 = run_mirror(c1, **rule), run_mirror(c2, rows=40, cols=50, stride=2, **rule)
        for _ in range(2):
            assert_same(run_device(h, c1, **rule), e1)
        assert_same(run_device(h, c2, rows=40, cols=50, stride=2, **rule), e2)
        assert_same(run_device(h, c1, **rule), e1)
        with pytest.raises(ValueError):
            run_device(h, case(views17, 301, 4), **rule)
        with pytest.raises(ValueError):
            run_device(h, case(views17, 300, 5), **rule)
    finally:
        h.close()


def test_host_side_refusals_leave_results_and_targets(ctx, ca, views17):
    c = case(views17, 100, 2)
    rule = dict(rounds=1, iterations=1)
    exp = run_mirror(c, **rule)
    assert_same(run_device(ca, c, **rule), exp)
    t = {k: dev(c[k]) for k in ("vertices", "normals", "colours", "surface", "depthinv")}
    result = torch.full((3 * 560,), 0x5A, dtype=torch.uint8, device="cuda")
    L, h = ca.L, ca._h
    k4 = (C.c_float * 4)(*K)
    good_p, good_r = dict(PRM, two_sided=0), dict(huber=16.0, damping=0.0, eps=1e-7, min_pairs=6, min_views=2, rounds=1, iterations=1, stride=1)

    def views(bad=None):
        arr = (CA.View * 2)()
        for v in range(2):
            R, tt = c["R"][v].copy(), c["t"][v].copy()
            ptrs = [t["colours"][v].data_ptr(), t["surface"][v].data_ptr(), t["depthinv"][v].data_ptr()]
            fixed = int(v == 0)
            if v == 1 and bad == "pose":
                R[0, 0] = np.nan
            if v == 1 and bad == "huge":
                tt[0] = 1e300
            if v == 1 and bad == "colour":
                ptrs[0] = None
            if v == 1 and bad == "surface":
                ptrs[1] += 2
            if v == 1 and bad == "depthinv":
                ptrs[2] += 1
            if v == 1 and bad == "fixed":
                fixed = 2
            arr[v] = CA.View(RC.View(Pose((C.c_double * 9)(*R.reshape(9)), (C.c_double * 3)(*tt)), *ptrs), fixed)
        return arr

    def call(handle=h, vertices=t["vertices"].data_ptr(), normals=t["normals"].data_ptr(), n=100, V=2, vw=None, k=k4, rows=ROWS, cols=COLS, p=None, r=None,
             res=result.data_ptr(), bad=None, no_params=False, no_rule=False):
        P, Rl = RC.Params(*[dict(good_p, **(p or {}))[f] for f in ("z_min", "z_max", "surface_tolerance", "measured_tolerance", "min_cos", "two_sided")]), \
            CA.Rule(*[dict(good_r, **(r or {}))[f] for f in ("huber", "damping", "eps", "min_pairs", "min_views", "rounds", "iterations", "stride")])
        return L.rgbid_colouralign_run(handle, vertices, normals, n, V, views(bad) if vw is None else vw, k, rows, cols, None if no_params else C.byref(P),
                                       None if no_rule else C.byref(Rl), res)

    nan, inf = float("nan"), float("inf")
    refused = [dict(handle=None), dict(vw=C.c_void_p()), dict(k=None), dict(no_params=True), dict(no_rule=True), dict(res=None), dict(res=result.data_ptr() + 4),
               dict(n=CAP_N + 1), dict(V=0), dict(V=-1), dict(V=CAP_V + 1), dict(rows=0), dict(cols=0), dict(rows=16385), dict(cols=16385),
               dict(vertices=None), dict(vertices=t["vertices"].data_ptr() + 2), dict(normals=t["normals"].data_ptr() + 1),
               dict(bad="pose"), dict(bad="huge"), dict(bad="colour"), dict(bad="surface"), dict(bad="depthinv"), dict(bad="fixed"),
               dict(k=(C.c_float * 4)(nan, 1, 1, 1)), dict(k=(C.c_float * 4)(0, 1, 1, 1)), dict(k=(C.c_float * 4)(1, 0, 1, 1)), dict(k=(C.c_float * 4)(1, 1, inf, 1))]
    refused += [dict(p=p) for p in (dict(z_min=0.0), dict(z_min=nan), dict(z_max=inf), dict(z_min=5.0), dict(surface_tolerance=-1.0), dict(surface_tolerance=nan),
                                    dict(measured_tolerance=inf), dict(min_cos=-0.1), dict(min_cos=1.5), dict(min_cos=nan), dict(two_sided=2))]
    refused += [dict(r=r) for r in (dict(huber=0.0), dict(huber=-1.0), dict(huber=nan), dict(huber=inf), dict(damping=-1.0), dict(damping=nan), dict(eps=0.0),
                                    dict(eps=nan), dict(eps=inf), dict(min_pairs=5), dict(min_views=1), dict(rounds=0), dict(iterations=0), dict(stride=0),
                                    dict(rounds=-1), dict(rounds=16, iterations=17), dict(rounds=257), dict(rounds=65536, iterations=65536))]
    for kw in refused:
        assert call(**kw) == -1, kw
    # nothing was written, and the last run's targets are still there
    ca.ctx.sync()
    assert (result == 0x5A).all()
    got = ca.targets()
    assert got["S"].cpu().numpy().view(np.uint64).tobytes() == exp["S"].tobytes() and got["used"].cpu().numpy().view(np.uint32).tobytes() == exp["used"].tobytes()
    assert call() == 0                                           # and the same call with nothing wrong is taken
    ca.ctx.sync()
    assert result[:2 * 560].cpu().numpy().view(CA.RESULT).tobytes() == exp["records"].tobytes() and (result[2 * 560:] == 0x5A).all()
    # the targets' own refusals
    S = torch.full((101,), -7, dtype=torch.int64, device="cuda")
    assert L.rgbid_colouralign_targets(h, S.data_ptr() + 4, None, None) == -1 and L.rgbid_colouralign_targets(h, None, S.data_ptr() + 4, None) == -1
    assert L.rgbid_colouralign_targets(h, None, None, S.data_ptr() + 2) == -1 and L.rgbid_colouralign_targets(h, None, None, None) == 0
    ca.ctx.sync()
    assert (S == -7).all()
    fresh = CA.ColourAligner(ctx, 10, 2)
    try:
        assert L.rgbid_colouralign_targets(fresh._h, None, None, None) == -1
        with pytest.raises(ValueError):
            fresh.targets()
        out = torch.full((5 * 6 * 3 + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        img = t["colours"][0]
        for kw in (dict(rows=0), dict(cols=0), dict(f=0), dict(f=17), dict(rows=3, f=4), dict(src=None), dict(dst=None), dict(rows=16385)):
            a = dict(dict(src=img.data_ptr(), rows=ROWS, cols=COLS, f=8, dst=out.data_ptr()), **kw)
            assert L.rgbid_colouralign_downscale(fresh._h, a["src"], a["rows"], a["cols"], a["f"], a["dst"]) == -1, kw
        ca.ctx.sync()
        assert (out == 0xA5).all()
    finally:
        fresh.close()
    # the binding refuses before the library is touched
    for kw in (dict(fixed=(2,)), dict(rounds=0), dict(huber=0.0), dict(min_views=1), dict(stride=0), dict(min_cos=2.0), dict(z_min=-1.0)):
        with pytest.raises(ValueError):
            ca.run(t["vertices"], c["R"], c["t"], K, ROWS, COLS, t["colours"], **kw)
    with pytest.raises(ValueError):
        ca.run(t["vertices"], c["R"], c["t"], K, ROWS, COLS, t["colours"][:1])
    with pytest.raises(ValueError):
        ca.run(t["vertices"].cpu(), c["R"], c["t"], K, ROWS, COLS, t["colours"])


def test_the_stage_timer(ca, views17):
    c = case(views17, 2000, 5)
    assert set(ca.timing(True)) == set(CA.STAGES)
    rule = dict(rounds=2, iterations=2)
    try:
        got = run_device(ca, c, **rule)
        ms = ca.timing(True)
        print("colour align stages (ms):", ms)
        assert all(0 < ms[k] < 1000 for k in CA.STAGES)
        assert_same(got, run_mirror(c, **rule))
    finally:
        ca.timing(False)
    run_device(ca, c, **rule)
    assert all(v == 0 for v in ca.timing(False).values())      # a run that was not recorded reads zero


def test_the_box_filter(ca):
    r = np.random.default_rng(4)
    img = r.integers(0, 256, (50, 67, 3)).astype(U8)
    img[:4, :4] = 255; img[4:8, :4] = 0
    d = dev(img)
    for f in (1, 2, 3, 4, 16):
        out = torch.full(((50 // f) * (67 // f) * 3 + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        got = ca.downscale(d, f)
        ca.ctx.sync()
        assert got.cpu().numpy().tobytes() == CM.box_filter(img, f).tobytes(), f
        assert C.c_int(ca.L.rgbid_colouralign_downscale(ca._h, d.data_ptr(), 50, 67, f, out.data_ptr())).value == 0
        ca.ctx.sync()
        assert out[:-1].cpu().numpy().tobytes() == CM.box_filter(img, f).tobytes() and int(out[-1]) == 0xA5
    for f in (0, 17, 51, 2.0, None):
        with pytest.raises(ValueError):
            ca.downscale(d, f)


def test_refine_keyframes_against_the_mirror(ctx):
    """the prototype's scene through the one-shot: every scale's records equal the mirror's when it is fed the device rasteriser's depth
    planes at that scale's starting poses; the refined poses are at least twice as close to the true ones"""
    sc = CM.scene(size=0.02, nx=40, ny=30)
    tri = CM.plane_triangles(40, 30)
    v, t = dev(sc["vertices"]), dev(tri.astype(np.int32))
    kfs = [dict(R=sc["Rp"][k], t=sc["tp"][k], colour=dev(sc["colours"][k]), frame=k) for k in range(len(sc["Rp"]))]
    kw = dict(rounds=3, iterations=2, surface_tolerance=0.05)
    timing = {}
    out, results, figures = CA.refine_keyframes(ctx, v, t, kfs, sc["K"], sc["rows"], sc["cols"], scales=(4, 2, 1), timing=timing, **kw)
    print("refine_keyframes stages (ms):", timing)
    assert set(timing) == {"raster", "target", "system", "solve"} and all(x > 0 for x in timing.values())

    def surface_of(R, tt, K_f, r_f, c_f):
        return RS.render_mesh(ctx, v, t, R, tt, K_f, r_f, c_f, outputs=("depth",))["depth"].cpu().numpy()

    R, tt, outs = CM.refine(sc["vertices"], sc["Rp"], sc["tp"], sc["K"], sc["rows"], sc["cols"], sc["colours"], scales=(4, 2, 1), surface_of=surface_of,
                            fixed=(0,), params=dict(CM.PARAMS, surface_tolerance=0.05, measured_tolerance=0.0), rounds=3, iterations=2)
    assert len(results) == len(figures) == 3 and [f["scale"] for f in figures] == [4, 2, 1]
    for res, o, fig in zip(results, outs, figures):
        assert res["records"].tobytes() == o["records"].tobytes()
        assert fig["used"].tobytes() == o["records"]["used"].tobytes()
        assert np.array_equal(fig["cost"], CM.cost_per_pair(o["records"]), equal_nan=True)
    assert all(k["R"].tobytes() == R[i].tobytes() and k["t"].tobytes() == tt[i].tobytes() and k["colour"] is kfs[i]["colour"] and k["frame"] == i
               for i, k in enumerate(out))
    assert all(k["R"].tobytes() == sc["Rp"][i].tobytes() and k["t"].tobytes() == sc["tp"][i].tobytes() for i, k in enumerate(kfs))   # the input is not touched
    err = lambda Rs, ts: np.array([CM.pixel_error(sc["vertices"], sc["K"], Rs[i], ts[i], sc["R"][i], sc["t"][i]) for i in range(1, len(Rs))])
    before, after = err(sc["Rp"], sc["tp"]), err(R, tt)
    print("pixel error before", before, "after", after)
    assert (after <= before / 2).all()
    lines = CA.figure_lines(figures, results)
    assert len(lines) == 3 and all("cost per pair" in l and "1 fixed" in l for l in lines)
    with pytest.raises(ValueError):
        CA.refine_keyframes(ctx, v, t, kfs, sc["K"], sc["rows"], sc["cols"], scales=(32,))
    with pytest.raises(ValueError):
        CA.refine_keyframes(ctx, v, t, [], sc["K"], sc["rows"], sc["cols"])
    with pytest.raises(ValueError):
        CA.refine_keyframes(ctx, v, t, [dict(k, colour=None) for k in kfs], sc["K"], sc["rows"], sc["cols"])


# ---- through the volume and the command line ----------------------------------------------------------------------------------------------
def synth_keyframes(n, rows, cols):
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.03, 0.05), rot_step_deg=(1.0, 2.0))
    d = seq["depth"].to(torch.float32)
    iD = torch.where(d > 0, 1000.0 / d, torch.zeros_like(d)).contiguous()
    return [dict(R=seq["R_wc"][k].cpu().numpy(), t=seq["t_wc"][k].cpu().numpy(), depthinv=iD[k].contiguous(), colour=seq["rgb"][k].contiguous())
            for k in range(n)]


def test_fuse_with_colour_align(ctx):
    """the geometry and the volume's figures keep their bytes; the colours are those of recolour_mesh at the refined poses"""
    rows, cols = 120, 160
    kfs = synth_keyframes(4, rows, cols)
    xyz = []
    for k in kfs:                                           # the cloud's box from the keyframes' own depth
        v, u = torch.meshgrid(torch.arange(rows, device="cuda"), torch.arange(cols, device="cuda"), indexing="ij")
        z = 1.0 / k["depthinv"].double()
        cam = torch.stack([(u - K_SMALL[2]) / K_SMALL[0] * z, (v - K_SMALL[3]) / K_SMALL[1] * z, z], -1).reshape(-1, 3)
        xyz.append(cam[torch.isfinite(cam).all(1)] @ torch.from_numpy(k["R"]).cuda().T + torch.from_numpy(k["t"]).cuda())
    xyz = torch.cat(xyz)
    lo, hi = xyz.min(0).values.cpu().numpy(), xyz.max(0).values.cpu().numpy()
    voxel = float(max(hi - lo + 0.4)) / 62
    args = dict(bounds=[*(lo - 0.2), *(hi + 0.2)], voxel=voxel, normals=True, return_volume=True, recolour="mean")
    plain = TS.fuse(ctx, kfs, K_SMALL, rows, cols, **args)
    assert plain[0].shape[0] > 300 and "colour_align" not in plain[4]
    opt = dict(scales=(2, 1), rounds=2, iterations=2)
    got = TS.fuse(ctx, kfs, K_SMALL, rows, cols, colour_align=opt, **args)
    assert all(got[i].cpu().numpy().tobytes() == plain[i].cpu().numpy().tobytes() for i in (0, 2, 3))
    al = got[4]["colour_align"]
    assert {k: x for k, x in got[4].items() if k not in ("colour_align", "recolour")} == {k: x for k, x in plain[4].items() if k != "recolour"}
    refined, results, figures = CA.refine_keyframes(ctx, plain[0], plain[2], kfs, K_SMALL, rows, cols, plain[3], surface_tolerance=2 * args["voxel"], **opt)
    assert all(a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes() for a, b in zip(al["keyframes"], refined))
    assert [f["scale"] for f in al["figures"]] == [2, 1] and int(al["results"][0]["status"][0]) == CA.FIXED
    raw = TS.fuse(ctx, kfs, K_SMALL, rows, cols, **dict(args, recolour=None))           # the extraction's own colours: what an unseen vertex keeps
    exp, _, _ = RC.recolour_mesh(ctx, plain[0], plain[2], refined, K_SMALL, rows, cols, plain[3], raw[1], "mean", 2 * args["voxel"], None)
    assert got[1].cpu().numpy().tobytes() == exp.cpu().numpy().tobytes() and (got[1] != plain[1]).any()
    assert any(int(s) in (CA.RUNNING, CA.CONVERGED) for s in al["results"][-1]["status"][1:])
    with pytest.raises(ValueError):
        TS.fuse(ctx, kfs, K_SMALL, rows, cols, colour_align=dict(scales=(0,)), **args)
    with pytest.raises(ValueError):
        TS.fuse(ctx, [dict(k, colour=None) for k in kfs], K_SMALL, rows, cols, colour_align={}, **dict(args, recolour=None))


def test_track_dataset_mesh_colour_align(ctx, tmp_path):
    """without the option every output keeps its bytes; with it the geometry of the PLY and of the OBJ does, the vertex colours and the
    atlas are sampled at the refined poses and one line per scale is added"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    recolour = ["--mesh-recolour", "mean", "--mesh-recolour-tolerance", "0.08"]
    said = {}
    for name, extra in (("plain", recolour),
                        ("aligned", recolour + ["--mesh-colour-align", "--mesh-colour-align-scales", "2,1", "--mesh-colour-align-rounds", "2"])):
        (tmp_path / name).mkdir()
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply"), "--mesh-voxel", "0.05", "--mesh-normals",
                                   "--mesh-texture", str(tmp_path / name / "tex.obj"), "--mesh-texture-tolerance", "0.08"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = [l.replace(f"{name}.ply", "plain.ply").replace(f"{name}/tex.obj", "plain/tex.obj") for l in r.stdout.splitlines() if "frames/s" not in l]
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_aligned.txt").read_bytes()
    added = [l for l in said["aligned"] if "mesh colour align: scale" in l]
    assert len(added) == 2 and "scale 2" in added[0] and "scale 1" in added[1] and all("cost per pair" in l for l in added)
    rest = [l for l in said["aligned"] if l not in added]
    sampled = lambda l: "mesh recolour" in l or "mesh texture" in l         # their pair counts are those of the poses they sample at
    assert [l for l in rest if not sampled(l)] == [l for l in said["plain"] if not sampled(l)]
    assert len([l for l in rest if sampled(l)]) == len([l for l in said["plain"] if sampled(l)]) == 2
    a, b = (TS.read_mesh_ply((tmp_path / f"{x}.ply").read_bytes()) for x in ("plain", "aligned"))
    assert all(a[i].tobytes() == b[i].tobytes() for i in (0, 2, 3)) and (a[1] != b[1]).any()
    # the textured mesh: the OBJ and its material keep their bytes, the atlas is baked from the refined poses
    from rgbid import texture as TX
    assert all((tmp_path / "plain" / f).read_bytes() == (tmp_path / "aligned" / f).read_bytes() for f in ("tex.obj", "tex.mtl"))
    oa, ob = (TX.read_obj(str(tmp_path / x / "tex.obj")) for x in ("plain", "aligned"))
    assert oa["atlas"].shape == ob["atlas"].shape and (oa["atlas"] != ob["atlas"]).any()
    for extra, word in ((["--mesh", str(tmp_path / "x.ply"), "--mesh-colour-align"], "--mesh-colour-align needs --mesh-recolour or --mesh-texture"),
                        (["--mesh", str(tmp_path / "x.ply")] + recolour + ["--mesh-colour-align-rounds", "2"], "need --mesh-colour-align")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr
