"""GPU tests of the recolouring stage (include/rgbid_recolour.h, csrc/kernels_recolour.hip, rgbid.recolour): colours, views_used,
best_view and the six counts per view byte for byte against the numpy restatement (tests/recolour_mirror.py), a canary element behind
every output; the cases of tests/test_cpu_recolour.py at the wave, block and chunk edges; both modes; every combination of optional
inputs; each output absent in turn and the colours in place; calls in every order on a handle of exact capacity; 20 000 random vertices
over 17 views with every class and every kind of bad value; an occlusion scene through the rasteriser; every host-side refusal; and
rgbid.tsdf.fuse and tools/track_dataset.py with the option."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import raster as RS, recolour as RC, synth, tsdf as TS
from tests import recolour_mirror as CM
from tests.test_cpu_recolour import BOUNDARIES, OPTIONAL, case, constant, mirror, random_case, two_view_case
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U8, U32 = np.float32, np.uint8, np.uint32
CAP_V = 20000
OUTPUTS = ("colours", "views_used", "best_view")
CANARY = {"colours": 0xA5, "views_used": -7, "best_view": -9}


@pytest.fixture(scope="module")
def rc(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh and an image of another size"""
    h = RC.Recolourer(ctx, CAP_V)
    yield h
    h.close()


def dev(a):
    if a is None:
        return None
    a = np.array(a, order="C")           # a copy: a broadcast array is not writable
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def add_views(rc, c, split=None, drop=(), vertices=None):
    """the case's views in calls of `split` views; -> the device tensors, which the caller keeps until the stream has run"""
    V = len(c["R"])
    step = V if split is None else split
    opt = {k: None if k in drop else dev(c[k]) for k in OPTIONAL}
    vertices, colours = dev(c["vertices"]) if vertices is None else vertices, dev(c["colours"])
    part = lambda x, a: None if x is None else x[a:a + step]
    for a in range(0, V, step):
        rc.add(vertices, c["R"][a:a + step], c["t"][a:a + step], c["K"], c["rows"], c["cols"], colours[a:a + step], part(opt["surface"], a),
               part(opt["depthinv"], a), opt["normals"], **c["params"])
    return vertices, colours, opt


def outputs_with_canary(n, names, colours_in=None):
    out = {}
    for o in names:
        shape = (n + 1, 3) if o == "colours" else (n + 1,)
        out[o] = torch.full(shape, CANARY[o], dtype=torch.uint8 if o == "colours" else torch.int32, device="cuda")
    if colours_in is not None and "colours" in out:
        out["colours"][:n] = colours_in
    return out


def assert_finished(rc, n, exp, mode, colours_in=None, names=OUTPUTS, inplace=False):
    """one finish into outputs with a canary element behind them: the requested outputs' bytes, the canaries, the counts per view"""
    names = [o for o in names if o != "best_view" or mode == "best"]
    cin = None if colours_in is None else dev(colours_in)
    out = outputs_with_canary(n, names, cin if inplace else None)
    rc.ctx.wait_torch_stream()
    rc.finish_into(out["colours"][:n] if inplace else cin, **{("colours_out" if o == "colours" else o): out[o][:n] for o in names})
    rc.ctx.sync()
    for o in names:
        got = out[o][:n].cpu().numpy()
        want = exp[o].view(np.int32) if exp[o].dtype == U32 else exp[o]
        assert got.tobytes() == want.tobytes(), (o, np.flatnonzero((got != want).reshape(n, -1).any(1))[:5])
        assert (out[o][n] == CANARY[o]).all(), o
    if len(exp["counts"]):
        got = np.array([[k[x] for x in CM.COUNTS] for k in rc.counts()], np.int64)
        assert (got == exp["counts"]).all(), (got, exp["counts"])


def assert_recoloured(rc, c, mode, split=None, colours_in=None, drop=(), names=OUTPUTS, inplace=False, exp=None):
    exp = mirror(c, mode, colours_in=colours_in, drop=drop) if exp is None else exp
    rc.begin(len(c["vertices"]), mode)
    held = add_views(rc, c, split, drop)
    assert_finished(rc, len(c["vertices"]), exp, mode, colours_in, names, inplace)
    del held
    return exp


def some_colours(n, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(U8)


@functools.lru_cache(maxsize=None)
def edge_case(n_v, V):
    c = random_case(n_v, V, seed=n_v + V)
    return c, {mode: mirror(c, mode, colours_in=some_colours(n_v)) for mode in ("mean", "best")}


@pytest.mark.parametrize("V", [1, 16, 17, 33])
@pytest.mark.parametrize("n_v", [0, 1, 63, 64, 65, 255, 256, 257])
def test_wave_block_and_chunk_edges(rc, n_v, V):
    c, exp = edge_case(n_v, V)
    for mode in ("mean", "best"):
        assert_recoloured(rc, c, mode, colours_in=some_colours(n_v), exp=exp[mode])


@pytest.mark.parametrize("name", sorted(BOUNDARIES))
def test_class_boundaries(rc, name):
    c, _ = BOUNDARIES[name]
    for mode in ("mean", "best"):
        assert_recoloured(rc, c, mode)


def test_hand_derived_cases(rc):
    img = np.array([[(10, 20, 30), (110, 120, 130)], [(50, 60, 70), (250, 240, 230)]], U8)[None]
    ramp = np.repeat((10 * np.arange(8, dtype=U8))[None, :, None], 3, 2)[None]
    ties = np.stack([constant((10, 20, 30)), constant((200, 210, 220)), constant((90, 90, 90))])
    for c, want in ((case([(0.25, 0.75, 1.0)], img), [[84, 90, 96]]), (case([(2.5, 0, 1), (652 / 256, 0, 1), (2.55, 0, 1), (2.3, 0, 1)], ramp), None),
                    (two_view_case(), None), (two_view_case(41), None), (case([(1.5, 1.5, 1.0), (np.nan, 0, 1)], ties), None)):
        for mode in ("mean", "best"):
            exp = assert_recoloured(rc, c, mode)
            assert want is None or exp["colours"].tolist() == want


def test_every_combination_of_inputs(rc):
    c = random_case(257, 17, seed=41)
    cin = some_colours(257, 9)
    for k in range(len(OPTIONAL) + 1):
        for drop in itertools.combinations(OPTIONAL, k):
            for mode in ("mean", "best"):
                for colours_in in (None, cin):
                    assert_recoloured(rc, c, mode, colours_in=colours_in, drop=drop)


def test_each_output_absent_in_turn_and_in_place(rc):
    c = random_case(300, 5, seed=43)
    cin = some_colours(300, 11)
    for mode in ("mean", "best"):
        exp = mirror(c, mode, colours_in=cin)
        assert (exp["views_used"] == 0).any() and (exp["views_used"] > 0).any()
        for k in (1, 2, 3):
            for names in itertools.combinations(OUTPUTS, k):
                assert_recoloured(rc, c, mode, colours_in=cin, names=names, exp=exp)
        assert_recoloured(rc, c, mode, colours_in=cin, inplace=True, exp=exp)
        out = rc.finish(dev(cin))                           # the same state once more, through the call that allocates
        assert sorted(out) == sorted(o for o in OUTPUTS if o != "best_view" or mode == "best")
        assert all(out[o].cpu().numpy().tobytes() == exp[o].tobytes() for o in out)
        rc.finish_into()                                    # no output at all: nothing is launched
        rc.ctx.sync()


def test_calls_in_every_order_on_exact_capacity(ctx):
    big, small = random_case(400, 17, seed=5), random_case(50, 3, 9, 11, seed=6)
    h = RC.Recolourer(ctx, 400)
    try:
        for mode in ("mean", "best"):
            whole = mirror(big, mode)
            h.begin(400, mode)
            held = [add_views(h, dict(big, R=big["R"][:16], t=big["t"][:16], colours=big["colours"][:16], surface=big["surface"][:16],
                                      depthinv=big["depthinv"][:16]))]
            first = mirror(dict(big, R=big["R"][:16], t=big["t"][:16], colours=big["colours"][:16], surface=big["surface"][:16],
                                depthinv=big["depthinv"][:16]), mode)
            assert_finished(h, 400, first, mode)
            assert_finished(h, 400, first, mode)            # finish changes nothing
            held.append(add_views(h, dict(big, R=big["R"][16:], t=big["t"][16:], colours=big["colours"][16:], surface=big["surface"][16:],
                                          depthinv=big["depthinv"][16:])))
            assert_finished(h, 400, whole, mode)            # views may follow a finish: the 17th has the global index 16
            assert h.counts(16, 1) == [dict(zip(CM.COUNTS, whole["counts"][16].tolist()))]
            for split in (1, 16):
                assert_recoloured(h, big, mode, split=split, exp=whole)
            assert_recoloured(h, small, mode)               # a second begin with another n_v and another image size
            assert_recoloured(h, big, mode, exp=whole)
            del held
        with pytest.raises(ValueError):
            h.begin(401)
        with pytest.raises(ValueError):
            add_views(h, random_case(399, 1, seed=1))
        assert_recoloured(h, big, "mean")
    finally:
        h.close()


def test_20000_random_vertices(rc):
    c = random_case(20000, 17, 48, 64, seed=78)
    cin = some_colours(20000, 13)
    for mode in ("mean", "best"):
        exp = mirror(c, mode, colours_in=cin)
        share = exp["counts"].sum(0) / exp["counts"].sum()
        print("fuzz:", dict(zip(CM.COUNTS, share.round(4).tolist())), "unseen", int((exp["views_used"] == 0).sum()), "twice", int((exp["views_used"] >= 2).sum()))
        assert (share >= 0.01).all() and (exp["views_used"] == 0).any() and (exp["views_used"] >= 2).any()
        assert not np.isfinite(c["vertices"]).all() and not np.isfinite(c["normals"]).all() and (c["normals"] == 0).all(1).any()
        for plane in (c["surface"], c["depthinv"]):
            assert np.isnan(plane).any() and np.isposinf(plane).any() and np.isneginf(plane).any() and (plane <= 0).any()
        rc.timing(True)
        assert_recoloured(rc, c, mode, colours_in=cin, exp=exp)
        ms = rc.timing(False)
        print("fuzz ms:", ms)
        assert all(v > 0 for v in ms.values())


def test_two_quads_hide_each_other(ctx, rc):
    """two 17 x 17 vertex quads over x, y in [-1, 1] at z = 2 and z = 3; view 0 looks along +z from the origin, view 1 along -z from
    z = 5: each view's nearer quad fills its 17 x 17 image exactly and hides the other one"""
    g = np.arange(17) / 8.0 - 1.0
    xy = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    verts = np.concatenate([np.concatenate([xy, np.full((289, 1), z)], 1) for z in (2.0, 3.0)]).astype(F)
    cell = np.array([(j * 17 + i, j * 17 + i + 1, (j + 1) * 17 + i + 1, (j + 1) * 17 + i) for j in range(16) for i in range(16)])
    tris = np.concatenate([cell[:, [0, 1, 2]], cell[:, [0, 2, 3]]])
    tris = np.concatenate([tris, tris + 289]).astype(U32)
    R, t = np.stack([np.eye(3), np.diag([-1.0, 1.0, -1.0])]), np.array([[0.0, 0, 0], [0, 0, 5.0]])
    K, front, back = (16.0, 16.0, 8.0, 8.0), (200, 100, 50), (20, 40, 61)
    img = np.stack([constant(front, 17, 17), constant(back, 17, 17)])
    depth = RS.render_mesh(ctx, dev(verts), dev(tris), R, t, K, 17, 17, outputs=("depth",))["depth"]
    assert torch.isfinite(depth).all() and (depth == 2.0).all()
    c = case(verts, img, K, R, t, surface=depth.cpu().numpy(), z_min=0.05, z_max=20.0, surface_tolerance=0.02)
    for mode in ("mean", "best"):
        exp = assert_recoloured(rc, c, mode)
        assert (exp["views_used"] == 1).all() and (exp["colours"][:289] == front).all() and (exp["colours"][289:] == back).all()
        assert exp["counts"].tolist() == [[0, 0, 289, 0, 0, 289]] * 2
    exp = assert_recoloured(rc, c, "mean", drop=("surface",))
    assert (exp["views_used"] == 2).all() and (exp["colours"] == (110, 70, 56)).all()      # (50 + 61) / 2 = 55.5 rounds up
    exp = assert_recoloured(rc, c, "best", drop=("surface",))
    assert (exp["colours"] == front).all() and (exp["best_view"] == 0).all()


def test_host_side_refusals_leave_state_and_outputs(rc):
    c = random_case(300, 3, 20, 30, seed=9)
    n, p0 = 300, c["params"]
    L = rc.L
    nan, inf = float("nan"), float("inf")
    for mode in ("mean", "best"):
        exp = mirror(c, mode)
        rc.begin(n, mode)
        v, colours, opt = add_views(rc, c)
        out = outputs_with_canary(n, OUTPUTS)
        p = {k: x.data_ptr() for k, x in dict(v=v, nr=opt["normals"], col=colours, sf=opt["surface"], iD=opt["depthinv"], **out).items()}

        def view(R=np.eye(3), t=(0, 0, 0), col=p["col"], sf=p["sf"], iD=p["iD"]):
            return RC.View(RC.Pose((C.c_double * 9)(*np.asarray(R, np.float64).reshape(9)), (C.c_double * 3)(*t)), col, sf, iD)

        def add(h=rc._h, v=p["v"], nr=p["nr"], nv=n, V=1, views=view(), K=c["K"], rows=20, cols=30, params=True, **kw):
            prm = RC.Params(*[kw.get(k, p0[k]) for k in ("z_min", "z_max", "surface_tolerance", "measured_tolerance", "min_cos")], kw.get("two_sided", 0))
            return L.rgbid_recolour_add(h, v, nr, nv, V, C.byref(views) if views is not None else None, (C.c_float * 4)(*K) if K is not None else None,
                                        rows, cols, C.byref(prm) if params else None)

        rc.ctx.wait_torch_stream()
        refusals = [dict(h=None), dict(views=None), dict(K=None), dict(params=False), dict(V=0), dict(V=-1), dict(V=RC.MAX_VIEWS - 2), dict(nv=n - 1),
                    dict(nv=n + 1), dict(nv=CAP_V + 1), dict(rows=0), dict(cols=0), dict(rows=RC.MAX_DIM + 1), dict(cols=RC.MAX_DIM + 1),
                    dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=nan), dict(z_max=inf), dict(z_min=3.0, z_max=2.0),
                    dict(surface_tolerance=-1e-9), dict(surface_tolerance=nan), dict(surface_tolerance=inf), dict(measured_tolerance=-1.0),
                    dict(measured_tolerance=nan), dict(measured_tolerance=inf), dict(min_cos=-1e-6), dict(min_cos=1.0001), dict(min_cos=nan),
                    dict(two_sided=2), dict(two_sided=-1),
                    dict(K=(nan, 1, 0, 0)), dict(K=(1, inf, 0, 0)), dict(K=(0, 1, 0, 0)), dict(K=(1, 0, 0, 0)), dict(K=(1, 1, nan, 0)), dict(K=(1, 1, 0, inf)),
                    dict(views=view(t=(nan, 0, 0))), dict(views=view(R=np.full((3, 3), inf))), dict(views=view(R=np.full((3, 3), 1e300))),
                    dict(views=view(t=(1e300, 0, 0))), dict(views=view(col=None)), dict(views=view(sf=p["sf"] + 2)), dict(views=view(iD=p["iD"] + 1)),
                    dict(v=None), dict(v=p["v"] + 2), dict(nr=p["nr"] + 1)]
        for kw in refusals:
            assert add(**kw) == -1, kw
        fin = lambda h=rc._h, cin=None, col=p["colours"], used=p["views_used"], best=p["best_view"] if mode == "best" else None: \
            L.rgbid_recolour_finish(h, cin, col, used, best)
        bad_finish = [dict(h=None), dict(used=p["views_used"] + 2), dict(best=p["best_view"] + 1)] + ([dict(best=p["best_view"])] if mode == "mean" else [])
        for kw in bad_finish:
            assert fin(**kw) == -1, kw
        assert L.rgbid_recolour_begin(rc._h, CAP_V + 1, 0) == -1 and L.rgbid_recolour_begin(rc._h, n, 2) == -1 and L.rgbid_recolour_begin(rc._h, n, -1) == -1
        cnt = (C.c_ulonglong * 24)()
        for first, V, o in ((0, 4, cnt), (-1, 1, cnt), (3, 1, cnt), (0, 0, cnt), (0, 3, None), (2, 2, cnt)):
            assert L.rgbid_recolour_counts(rc._h, first, V, o) == -1, (first, V)
        rc.ctx.sync()
        assert all((out[o] == CANARY[o]).all() for o in out)
        assert rc.views == 3 and L.rgbid_recolour_counts(rc._h, 0, 3, cnt) == 0 and list(cnt[:18]) == exp["counts"].reshape(-1).tolist()
        assert_finished(rc, n, exp, mode)                   # the state is what the three views left
    fresh = RC.Recolourer(rc.ctx, 10)
    try:
        assert L.rgbid_recolour_finish(fresh._h, None, None, None, None) == -1 and L.rgbid_recolour_counts(fresh._h, 0, 1, cnt) == -1      # no begin
        prm = RC.Params(0.5, 4.0, 0.1, 0.1, 0.2, 0)
        assert L.rgbid_recolour_add(fresh._h, p["v"], None, 10, 1, C.byref(view()), (C.c_float * 4)(*c["K"]), 20, 30, C.byref(prm)) == -1
        for f in (lambda: fresh.add(v, c["R"], c["t"], c["K"], 20, 30, colours), fresh.finish, fresh.finish_into):
            with pytest.raises(ValueError):
                f()
    finally:
        fresh.close()
    for cap in (0, (1 << 31) + 1, 2.0):
        with pytest.raises(ValueError):
            RC.Recolourer(rc.ctx, cap)
    rc.begin(n, "mean")
    v, colours = dev(c["vertices"]), dev(c["colours"])
    good = dict(R=c["R"], t=c["t"], K=c["K"], rows=20, cols=30, colours=colours)
    for kw in (dict(rows=21), dict(colours=colours[:2]), dict(surface=dev(c["surface"])[:, :19]), dict(depthinv=dev(c["depthinv"]).double()),
               dict(normals=dev(c["normals"])[:-1]), dict(z_min=0), dict(min_cos=2), dict(surface_tolerance=-1), dict(two_sided="no"), dict(K=(0, 1, 0, 0))):
        with pytest.raises(ValueError):                     # the Python checks come first
            rc.add(v, **dict(good, **kw))
    with pytest.raises(ValueError):
        rc.add(v[:-1], **good)
    with pytest.raises(ValueError):
        rc.finish_into(best_view=torch.zeros(n, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        rc.counts()
    assert rc.views == 0


# ---- through the volume and the command line ----------------------------------------------------------------------------------------------
def synth_keyframes(n, rows, cols):
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.03, 0.05), rot_step_deg=(1.0, 2.0))
    d = seq["depth"].to(torch.float32)
    iD = torch.where(d > 0, 1000.0 / d, torch.zeros_like(d)).contiguous()
    return [dict(R=seq["R_wc"][k].cpu().numpy(), t=seq["t_wc"][k].cpu().numpy(), depthinv=iD[k].contiguous(), colour=seq["rgb"][k].contiguous())
            for k in range(n)]


def test_fuse_with_recolour(ctx):
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
    args = dict(bounds=[*(lo - 0.2), *(hi + 0.2)], voxel=voxel, normals=True, return_volume=True, simplify=2 * voxel, smooth=2)
    plain = TS.fuse(ctx, kfs, K_SMALL, rows, cols, **args)
    info = plain[4]
    assert max(info["nx"], info["ny"], info["nz"]) <= 64 and plain[0].shape[0] > 500 and "recolour" not in info
    for mode in ("mean", "best"):
        got = TS.fuse(ctx, kfs, K_SMALL, rows, cols, recolour=mode, **args)
        assert all(got[i].cpu().numpy().tobytes() == plain[i].cpu().numpy().tobytes() for i in (0, 2, 3))
        v, t, nrm = (plain[i] for i in (0, 2, 3))
        R, tw = np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs])
        depth = RS.render_mesh(ctx, v, t, R, tw, K_SMALL, rows, cols, outputs=("depth",))["depth"].cpu().numpy()
        exp = CM.recolour_numpy(v.cpu().numpy(), R, tw, K_SMALL, rows, cols, [k["colour"].cpu().numpy() for k in kfs], mode, plain[1].cpu().numpy(),
                                surface=depth, normals=nrm.cpu().numpy(), z_min=0.05, z_max=20.0, surface_tolerance=2.0 * voxel, measured_tolerance=0.0,
                                min_cos=0.2, two_sided=False)
        assert got[1].cpu().numpy().tobytes() == exp["colours"].tobytes()
        rec = got[4]["recolour"]
        print("fuse recolour:", rec)
        assert rec["mode"] == mode and rec["vertices"] == v.shape[0] and rec["coloured"] == int((exp["views_used"] > 0).sum()) > v.shape[0] // 2
        assert [rec[k] for k in CM.COUNTS] == exp["counts"].sum(0).tolist() and (got[1] != plain[1]).any()
        assert {k: x for k, x in got[4].items() if k != "recolour"} == info
    with pytest.raises(ValueError):
        TS.fuse(ctx, [dict(k, colour=None) for k in kfs], K_SMALL, rows, cols, recolour="mean", **args)
    with pytest.raises(ValueError):
        TS.fuse(ctx, kfs, K_SMALL, rows, cols, recolour="median", **args)
    with pytest.raises(ValueError):
        TS.fuse(ctx, kfs, K_SMALL, rows, cols, recolour_tolerance=0.1, **args)


def test_track_dataset_mesh_recolour(ctx, tmp_path):
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("best", ["--mesh-recolour", "best", "--mesh-recolour-tolerance", "0.08"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply"), "--mesh-voxel", "0.05", "--mesh-normals"]
                           + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = [l.replace("best.ply", "plain.ply") for l in r.stdout.splitlines() if "frames/s" not in l]
    added = [l for l in said["best"] if "mesh recolour (best)" in l]
    assert len(added) == 1 and [l for l in said["best"] if l not in added] == said["plain"]
    words = added[0].split()
    coloured, vertices = int(words[words.index("of") - 1]), int(words[words.index("of") + 1])
    assert all(f" {k}" in added[0] for k in CM.COUNTS)
    a, b = (TS.read_mesh_ply((tmp_path / f"{x}.ply").read_bytes()) for x in ("plain", "best"))
    assert all(a[i].tobytes() == b[i].tobytes() for i in (0, 2, 3)) and len(a[0]) == vertices and 0 < coloured <= vertices
    assert (a[1] != b[1]).any()
    r = subprocess.run(base + ["--mesh-recolour", "mean"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--mesh-recolour needs --mesh" in r.stderr
