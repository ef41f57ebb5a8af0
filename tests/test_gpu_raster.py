"""GPU tests of the mesh rasteriser (include/rgbid_raster.h, csrc/kernels_raster.hip, rgbid.raster): every plane and the six counts per
view byte for byte against the numpy restatement (tests/raster_mirror.py), a canary view behind every output; the meshes of
tests/test_cpu_raster.py at 1, 16 and 17 views on one handle; every combination of outputs; boxes of exactly SMALL_BOX and SMALL_BOX + 1
pixels; 0, 1 and 257 triangles on the large path; a triangle that fills 640 x 480; boxes that start and end inside a tile and on its
edges; counts either side of a block; 20 000 random triangles with vertices that are not finite; calls in every order on a handle of
exact capacities; a bad index; every host-side refusal; and rgbid.tsdf's meshes, a tracked run and tools/track_dataset.py.

The six counts do not say which kernel drew a triangle, but the header's SMALL_BOX does: the fragments of a triangle whose box holds more
pixels reach the counts and the planes through k_rast_large only, those of a smaller one through k_rast_setup only, so a case whose
counts and planes hold both kinds has run both paths."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import raster as RS, render as RD, sequence, synth, tsdf as TS, tum
from tests import raster_mirror as XM
from tests import tsdf_mirror as TM
from tests.test_cpu_raster import CASES, attributes, case, flat, mirror, random_case, with_views
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
CAP_V, CAP_T, CAP_PIX = 3001, 20001, 640 * 480
ALL = ("index", "depth", "colour", "normal")
CANARY = {"index": -7, "depth": 7.5, "colour": 0xA5, "normal": -3.25}


@pytest.fixture(scope="module")
def rs(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh and an image of another size"""
    h = RS.Rasteriser(ctx, CAP_V, CAP_T, CAP_PIX)
    yield h
    h.close()


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def raw(x):
    return x.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def expected(name, V):
    """the mirror's planes of a case of the CPU file at V views, computed once"""
    c = with_views(CASES[name](), V)
    return c, mirror(c)


def assert_rendered(rs, c, exp, outputs=ALL, colours=True, normals=True):
    """one call into planes with a canary view behind them: the requested planes' bytes, the canaries, the six counts per view"""
    V, rows, cols = len(c["R"]), c["rows"], c["cols"]
    shapes = RS.plane_shapes(V + 1, rows, cols)
    planes = {o: torch.full(shapes[o][0], CANARY[o], dtype=shapes[o][1], device="cuda") for o in outputs}
    mesh = [dev(c["vertices"]), dev(c["triangles"])]
    rs.ctx.wait_torch_stream()
    rs.render_into(*mesh, c["R"], c["t"], c["K"], rows, cols, dev(c["colours"]) if colours else None, dev(c["normals"]) if normals else None,
                   c["z_min"], c["z_max"], **{o: planes[o][:V] for o in outputs})
    rs.ctx.sync()
    for o in outputs:
        got = planes[o][:V].cpu().numpy()
        same = got.tobytes() == exp[o].tobytes()
        assert same, (o, np.argwhere(got.view(np.uint8).reshape(V, -1) != exp[o].view(np.uint8).reshape(V, -1))[:5])
        assert (planes[o][V] == CANARY[o]).all(), o
    got = np.array([[n[k] for k in XM.COUNTS] for n in rs.counts()], np.int64)
    assert (got == exp["counts"]).all(), (got, exp["counts"])


@pytest.mark.parametrize("V", [1, 16, 17])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_cases_against_the_mirror(rs, name, V):
    c, exp = expected(name, V)
    assert_rendered(rs, c, exp)


def test_every_combination_of_outputs(rs):
    c, exp = expected("crossing", 2)
    for k in range(1, 5):
        for outs in itertools.combinations(ALL, k):
            assert_rendered(rs, c, exp, outs, colours="colour" in outs, normals="normal" in outs)
    got = rs.render(dev(c["vertices"]), dev(c["triangles"]), c["R"], c["t"], c["K"], c["rows"], c["cols"], dev(c["colours"]), dev(c["normals"]),
                    c["z_min"], c["z_max"], outputs=ALL)
    assert all(raw(got[o]) == exp[o].tobytes() for o in ALL) and got["index"].dtype == torch.int32 and (got["index"] == -1).any()
    one = RS.render_mesh(rs.ctx, dev(c["vertices"]), dev(c["triangles"]), c["R"], c["t"], c["K"], c["rows"], c["cols"], z_min=c["z_min"],
                         z_max=c["z_max"], outputs=("depth",))
    assert list(one) == ["depth"] and raw(one["depth"]) == exp["depth"].tobytes()


def rectangles(boxes, rows, cols, seed=21):
    """two triangles per pixel box (x0, y0, x1, y1), inclusive: the rectangle reaches a quarter pixel beyond the box's outer centres, so each
    triangle's box is the rectangle's and a box of one row or one column is no degenerate triangle"""
    pts, tris = [], []
    for x0, y0, x1, y1 in boxes:
        k = len(pts)
        pts += [(x0 - 0.25, y0 - 0.25), (x1 + 0.25, y0 - 0.25), (x1 + 0.25, y1 + 0.25), (x0 - 0.25, y1 + 0.25)]
        tris += [(k, k + 1, k + 2), (k, k + 2, k + 3)]
    col, nr = attributes(len(pts), seed)
    return case(flat(pts), tris, rows, cols, colours=col, normals=nr)


def test_boxes_either_side_of_the_small_box(rs):
    """boxes of exactly SMALL_BOX and SMALL_BOX + 1 pixels, as rows and as rectangles; the fragments of each kind are in the counts"""
    s = RS.SMALL_BOX
    assert s == 16
    c = rectangles([(1, 1, s, 1), (1, 3, s + 1, 3), (1, 5, 4, 8), (8, 5, 8, 5 + s), (12, 5, 12 + 3, 5 + 3), (20, 5, 20 + 4, 5 + 3)], 24, 32)
    exp = mirror(c)
    boxes = [s, s + 1, s, s + 1, s, 20]
    assert exp["counts"][0].tolist()[:4] == [0, 0, 0, 12] and exp["counts"][0][5] == sum(boxes)
    # twice: the 4 diagonal centres of each square, and the middle centre of each box of 17 (its diagonal passes (8.25, 0.25) of 16.5 x 0.5)
    assert exp["counts"][0][4] == sum(boxes) + 4 + 4 + 1 + 1
    assert_rendered(rs, c, exp)
    only_small = rectangles([(1, 1, s, 1), (1, 5, 4, 8)], 24, 32)
    assert_rendered(rs, only_small, mirror(only_small))


@pytest.mark.parametrize("n_large", [0, 1, 257])
def test_large_triangles(rs, n_large):
    """n_large rectangles of 5 x 5 pixels among small ones, over 2 views"""
    rng = np.random.default_rng(n_large)
    boxes = [(int(x), int(y), int(x) + 4, int(y) + 4) for x, y in zip(rng.integers(-3, 150, (n_large + 1) // 2), rng.integers(-3, 100, (n_large + 1) // 2))]
    boxes += [(int(x), int(y), int(x) + 2, int(y) + 1) for x, y in zip(rng.integers(0, 150, 40), rng.integers(0, 100, 40))]
    c = rectangles(boxes, 104, 156)
    c["triangles"] = c["triangles"][n_large % 2:]                                # an odd number: the first rectangle loses a half
    c = with_views(c, 2)
    exp = mirror(c)
    assert_rendered(rs, c, exp)


def test_one_triangle_fills_640_x_480(rs):
    col, nr = attributes(3, 31)
    c = case([(-2000, -1000, 1), (4000, -1000, 2), (-2000, 6000, 4)], [(0, 1, 2)], 480, 640, colours=col, normals=nr)
    exp = mirror(c)
    assert exp["counts"][0].tolist() == [0, 0, 0, 1, 480 * 640, 480 * 640]
    rs.timing(True)
    assert_rendered(rs, c, exp)
    ms = rs.timing(False)
    print("one triangle over 640 x 480, ms:", ms)
    assert all(v > 0 for v in ms.values())


def test_boxes_inside_and_on_the_edges_of_tiles(rs):
    t = RS.TILE
    assert t == 8
    boxes = [(t, t, 2 * t - 1, 2 * t - 1 + t), (t + 1, 3 * t + 1, 2 * t - 2, 4 * t + 4), (t - 1, 6 * t - 1, 2 * t, 7 * t), (3 * t + 3, 1, 5 * t + 4, 3 * t + 2),
              (0, 0, t - 1, t - 1), (3 * t, 5 * t, 6 * t - 1, 6 * t - 1), (5 * t + 2, 3 * t + 5, 5 * t + 4, 6 * t)]
    c = with_views(rectangles(boxes, 8 * t + 3, 7 * t + 5), 3)
    assert_rendered(rs, c, mirror(c))


@pytest.mark.parametrize("n", [255, 256, 257])
def test_counts_either_side_of_a_block(rs, n):
    for c in (random_case(n, 300, 20, 30, n, bad=4), random_case(90, n, 20, 30, n + 1000, bad=4)):
        assert_rendered(rs, c, mirror(c))


def test_20000_random_triangles(rs):
    c = random_case(3000, 20000, 120, 160, 77, bad=40)
    exp = mirror(c)
    n = dict(zip(XM.COUNTS, exp["counts"][0].tolist()))
    print("random mesh:", n)
    assert n["gated"] > 500 and n["degenerate"] > 0 and n["empty_box"] > 100 and n["drawn"] > 5000 and n["fragments"] > n["pixels"] > 10000
    assert_rendered(rs, c, exp)


def test_calls_in_every_order_on_exact_capacities(ctx):
    big, small, wall = random_case(400, 900, 30, 40, 5, bad=4), random_case(50, 60, 9, 11, 6), with_views(CASES["wall"](), 1)
    empty = dict(big, vertices=np.zeros((0, 3), F), triangles=np.zeros((0, 3), U32), colours=np.zeros((0, 3), np.uint8), normals=np.zeros((0, 3), F))
    no_tri = dict(big, triangles=np.zeros((0, 3), U32))
    h = RS.Rasteriser(ctx, 400, 900, 48 * 64)
    try:
        for c in (big, small, empty, wall, big, no_tri, small, with_views(small, 17), big):
            exp = mirror(c)
            if not len(c["triangles"]):
                assert (exp["index"] == XM.EMPTY).all() and (exp["counts"] == 0).all()
            assert_rendered(h, c, exp)
        for bad in (random_case(401, 900, 30, 40, 5), random_case(400, 901, 30, 40, 5), dict(big, rows=48, cols=65)):
            with pytest.raises(ValueError):
                assert_rendered(h, bad, None)
        assert_rendered(h, big, mirror(big))
    finally:
        h.close()


def test_a_bad_index_ends_the_call(rs):
    c = random_case(300, 700, 20, 30, 9)
    exp = mirror(c)
    for at, corner in ((0, 0), (350, 1), (699, 2)):
        bad = dict(c, triangles=c["triangles"].copy())
        bad["triangles"][at, corner] = 300
        with pytest.raises(Exception, match="rgbid error -1"):
            assert_rendered(rs, bad, exp)
        with pytest.raises(ValueError):
            rs.counts()
        planes = {o: torch.full(s, CANARY[o], dtype=d, device="cuda") for o, (s, d) in RS.plane_shapes(1, 20, 30).items()}
        with pytest.raises(Exception, match="rgbid error -1"):
            rs.render_into(dev(bad["vertices"]), dev(bad["triangles"]), c["R"], c["t"], c["K"], 20, 30, dev(c["colours"]), dev(c["normals"]),
                           c["z_min"], c["z_max"], **planes)
        rs.ctx.sync()
        assert all((planes[o] == CANARY[o]).all() for o in planes)              # nothing else was launched
        assert_rendered(rs, c, exp)                                             # the next valid call is correct


def test_host_side_refusals_leave_the_outputs(rs):
    c = random_case(300, 700, 20, 30, 9)
    exp = mirror(c)
    L = rs.L
    v, t, col, nr = dev(c["vertices"]), dev(c["triangles"]), dev(c["colours"]), dev(c["normals"])
    planes = {o: torch.full(s, CANARY[o], dtype=d, device="cuda") for o, (s, d) in RS.plane_shapes(1, 20, 30).items()}
    pose = RS.Pose((C.c_double * 9)(*np.eye(3).reshape(9)), (C.c_double * 3)(0, 0, 0))
    p = {k: x.data_ptr() for k, x in dict(v=v, t=t, col=col, nr=nr, **planes).items()}
    nan, inf = float("nan"), float("inf")

    def call(h=rs._h, v=p["v"], nv=300, t=p["t"], nt=700, col=p["col"], nr=p["nr"], V=1, poses=pose, K=c["K"], rows=20, cols=30, z_min=0.5, z_max=4.0,
             index=p["index"], depth=p["depth"], colour=p["colour"], normal=p["normal"]):
        k = (C.c_float * 4)(*K) if K is not None else None
        return L.rgbid_raster_views(h, v, nv, t, nt, col, nr, V, C.byref(poses) if poses is not None else None, k, rows, cols, z_min, z_max, index,
                                    depth, colour, normal)

    def posed(R=np.eye(3), t=(0, 0, 0)):
        return RS.Pose((C.c_double * 9)(*np.asarray(R, np.float64).reshape(9)), (C.c_double * 3)(*t))

    rs.ctx.wait_torch_stream()
    refusals = [dict(h=None), dict(poses=None), dict(K=None), dict(V=0), dict(V=-1), dict(V=RS.MAX_VIEWS + 1), dict(rows=0), dict(cols=0),
                dict(rows=RS.MAX_DIM + 1), dict(cols=RS.MAX_DIM + 1), dict(rows=480, cols=641), dict(V=CAP_PIX // 600 + 1),
                dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=nan), dict(z_max=inf), dict(z_min=3.0, z_max=2.0),
                dict(K=(nan, 1, 0, 0)), dict(K=(1, inf, 0, 0)), dict(K=(0, 1, 0, 0)), dict(K=(1, 0, 0, 0)), dict(K=(1, 1, nan, 0)), dict(K=(1, 1, 0, inf)),
                dict(poses=posed(t=(nan, 0, 0))), dict(poses=posed(R=np.full((3, 3), inf))), dict(poses=posed(R=np.full((3, 3), 1e300))),
                dict(poses=posed(t=(1e300, 0, 0))),
                dict(nv=CAP_V + 1), dict(nt=CAP_T + 1), dict(v=None), dict(t=None), dict(v=p["v"] + 2), dict(t=p["t"] + 1), dict(nv=0),
                dict(nr=p["nr"] + 2), dict(index=p["index"] + 1), dict(depth=p["depth"] + 2), dict(normal=p["normal"] + 3),
                dict(col=None), dict(nr=None)]
    for kw in refusals:
        assert call(**kw) == -1, kw
    rs.ctx.sync()
    assert all((planes[o] == CANARY[o]).all() for o in planes)
    assert call(col=None, colour=None) == 0 and call(nr=None, normal=None) == 0 and call() == 0      # an attribute nobody asks for may be absent
    rs.ctx.sync()
    assert all(raw(planes[o]) == exp[o].tobytes() for o in planes)
    out = (C.c_ulonglong * 12)()
    assert L.rgbid_raster_counts(rs._h, 2, out) == -1 and L.rgbid_raster_counts(rs._h, 1, None) == -1 and L.rgbid_raster_counts(rs._h, 1, out) == 0
    assert list(out[:6]) == exp["counts"][0].tolist()
    for caps in ((0, 10, 100), (10, 0, 100), (10, 10, 0), (10, 1 << 31, 100)):
        with pytest.raises(Exception):
            RS.Rasteriser(rs.ctx, *caps)
    for kw in (dict(outputs=("normal",), normals=None), dict(outputs=("colour",), colours=None), dict(rows=RS.MAX_DIM + 1), dict(z_min=0)):
        args = dict(dict(R=c["R"], t=c["t"], K=c["K"], rows=20, cols=30, colours=col, normals=nr), **kw)
        with pytest.raises(ValueError):                     # the Python checks come first
            rs.render(v, t, **args)
    with pytest.raises(ValueError):
        rs.render(v, t[:, :2], c["R"], c["t"], c["K"], 20, 30)
    with pytest.raises(ValueError):
        rs.render(v, t, c["R"], c["t"], c["K"], 20, 30, colours=col[:-1])
    assert_rendered(rs, c, exp)


# ---- through the volume, a tracked run and the command line -----------------------------------------------------------------------------
def host_mesh(v, c, t, n=None):
    return v.cpu().numpy(), t.cpu().numpy().view(U32), None if c is None else c.cpu().numpy(), None if n is None else n.cpu().numpy()


def test_volume_extract_then_render_mesh(ctx):
    """a large and a small sphere in 128 x 64 x 64 voxels through Volume.extract with every clean-up option, rasterised from two poses,
    against the mirror over the same tensors"""
    m = TM.Volume(128, 64, 64, (0.0, 0.0, 0.0), 0.05, 0.2)
    big, W = TM.sphere_state(m, (3.2, 1.6, 1.6), 1.5)
    small, _ = TM.sphere_state(m, (0.4, 0.4, 0.4), 0.25)
    vol = TS.Volume(ctx, m.n, 1, colour=False)
    vol.configure(128, 64, 64, [0.0, 0.0, 0.0], 0.05, 0.2)
    vol.set_state(torch.from_numpy(np.minimum(big, small)).cuda(), torch.from_numpy(W.view(np.int32)).cuda())
    v, c, t, n = vol.extract(1, normals=True, min_component=5000, simplify=0.2, smooth=dict(iterations=5, pin_boundary=True))
    vol.close()
    assert t.shape[0] > 500
    R, tw = np.stack([np.eye(3), np.eye(3)]), np.array([[3.2, 1.6, -2.5], [2.9, 1.8, -1.0]])
    K, rows, cols = (60.0, 58.0, 31.5, 23.5), 48, 64
    got = RS.render_mesh(ctx, v, t, R, tw, K, rows, cols, c, n, z_min=0.3, z_max=8.0, outputs=("index", "depth", "colour", "normal"))
    hv, ht, hc, hn = host_mesh(v, c, t, n)
    exp = XM.raster_numpy(hv, ht, R, tw, K, rows, cols, hc, hn, 0.3, 8.0)
    assert all(raw(got[o]) == exp[o].tobytes() for o in got) and (exp["counts"][:, 5] > 500).all()
    print("two spheres, cleaned up:", exp["counts"].tolist())


def test_mesh_agreement_of_a_tracked_run(ctx):
    """the tracked run of tests/test_gpu_tsdf.py through fuse and mesh_agreement, beside surface_agreement.  The figures are printed and
    asserted only against the same statistic over the mirror's planes."""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                         keyframe_colour=True)
    v, c, t, info, vol = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, keep_volume=True,
                                 simplify=0.08, smooth=5)
    try:
        surface = TS.surface_agreement(vol, pc.keyframes, K_SMALL, rows, cols)
    finally:
        vol.close()
    figures = RS.mesh_agreement(ctx, v, t, pc.keyframes, K_SMALL, rows, cols)
    hv, ht, _, _ = host_mesh(v, c, t)
    want = []
    for kf in pc.keyframes:
        d = XM.raster_numpy(hv, ht, kf["R"], kf["t"], K_SMALL, rows, cols)["depth"][0]
        want.append(RS.agreement_of(torch.from_numpy(d), kf["depthinv"]))
    print("mesh agreement:", figures, RD.agreement_summary(figures), "\nsurface agreement:", surface, RD.agreement_summary(surface))
    assert figures == want and len(figures) == len(pc.keyframes) and all(f["pixels"] > 1000 for f in figures)


def test_track_dataset_mesh_raster_options(ctx, tmp_path):
    """without the new options PLY, trajectory and printed lines are what they are today; with them the same bytes, the PNGs hold exactly
    render_mesh's planes and the check's lines stand after the volume's"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    views, said = tmp_path / "views", {}
    clean = ["--mesh-voxel", "0.05", "--mesh-min-weight", "2", "--mesh-normals", "--mesh-simplify", "0.1", "--mesh-smooth", "3", "--mesh-render-check"]
    for name, extra in (("plain", []), ("raster", ["--mesh-raster", str(views), "--mesh-raster-check"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply")] + clean + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = [l.replace("raster.ply", "plain.ply") for l in r.stdout.splitlines() if "frames/s" not in l]
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_raster.txt").read_bytes()
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "raster.ply").read_bytes()
    added = [l for l in said["raster"] if "mesh raster" in l or "rasterised views" in l]
    assert [l for l in said["raster"] if l not in added] == said["plain"] and len(added) == len(said["raster"]) - len(said["plain"]) > 2
    at = [i for i, l in enumerate(said["raster"]) if "mesh render check" in l or "mesh raster check" in l]
    assert at == list(range(at[0], at[0] + len(at))) and "mesh render check" in said["raster"][at[0]]   # the two tables one after the other
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True, keyframe_colour=True)
    v, c, t, nrm = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, normals=True, simplify=0.1, smooth=3)
    assert (tmp_path / "plain.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t, nrm)
    want = RS.render_mesh(ctx, v, t, np.stack([k["R"] for k in pc.keyframes]), np.stack([k["t"] for k in pc.keyframes]), K_SMALL, rows, cols, c, nrm,
                          outputs=("depth", "colour", "normal"))
    assert len(list(views.iterdir())) == 3 * len(pc.keyframes)
    for i in range(len(pc.keyframes)):
        assert np.array_equal(tum.read_png(str(views / f"mesh_{i:04d}.png")), want["colour"][i].cpu().numpy()), i
        assert np.array_equal(tum.read_png(str(views / f"mesh_{i:04d}_depth.png")), RD.depth_png(want["depth"][i])), i
        assert np.array_equal(tum.read_png(str(views / f"mesh_{i:04d}_shaded.png")), TS.shade(want["normal"][i])), i
    figures = RS.mesh_agreement(ctx, v, t, pc.keyframes, K_SMALL, rows, cols)
    run = RD.agreement_summary(figures)
    assert (f"mesh raster check: {len(figures)} keyframes, {run['pixels']} pixels, median of medians {run['median']:.6f} m, "
            f"largest 90 % {run['p90']:.6f} m") in "\n".join(said["raster"])
    assert sum("mesh raster check: keyframe" in l for l in said["raster"]) == len(figures)
