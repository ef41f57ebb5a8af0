"""GPU tests of the texturing stage (include/rgbid_texture.h, csrc/kernels_texture.hip, rgbid.texture): atlas, views_used, best_view, uv
and the six counts per view byte for byte against the numpy restatement (tests/texture_mirror.py), a canary behind every output; meshes
of 0 to 129 triangles at patch sizes whose tiles lie below, astride, on and above a wave, three atlas widths, view counts around the
chunk of 16, both modes; the hand and boundary cases of tests/test_cpu_texture.py; every combination of optional inputs; each output
absent in turn; calls in every order on a handle of exact capacity; a mixed scene with every class; an occlusion scene through the
rasteriser; every host-side refusal; texture_mesh and tools/track_dataset.py with the options."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import raster as RS, recolour as RC, synth, texture as TX, tsdf as TS
from tests import recolour_mirror as CM
from tests import texture_mirror as TM
from tests.test_cpu_recolour import OPTIONAL
from tests.test_cpu_texture import HAND_BYTES, QUAD, hand_case, mesh_case, mirror, ramp_image, random_mesh_case
from tests.test_gpu_cloud import K_SMALL, write_tum_folder
from tests.test_gpu_recolour import synth_keyframes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U8, U32 = np.float32, np.uint8, np.uint32
CAP_T, CAP_SLOTS = 2100, 1 << 17
OUTPUTS = TX.OUTPUTS
CANARY = {"atlas": 0xA5, "views_used": -7, "best_view": -9}
UV_CANARY = -5.0


@pytest.fixture(scope="module")
def tx(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh, a layout and an image of another size"""
    h = TX.Texturer(ctx, CAP_T, CAP_SLOTS)
    yield h
    h.close()


def dev(a):
    if a is None:
        return None
    a = np.array(a, order="C")           # a copy: a broadcast array is not writable
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def add_views(tx, c, split=None, drop=(), mesh=None):
    """the case's views in calls of `split` views; -> the device tensors, which the caller keeps until the stream has run"""
    V = len(c["R"])
    step = max(V, 1) if split is None else split
    opt = {k: None if k in drop else dev(c[k]) for k in OPTIONAL}
    (vertices, triangles), colours = (dev(c["vertices"]), dev(c["triangles"])) if mesh is None else mesh, dev(c["colours"])
    part = lambda x, a: None if x is None else x[a:a + step]
    for a in range(0, V, step):
        tx.add(vertices, triangles, c["R"][a:a + step], c["t"][a:a + step], c["K"], c["rows"], c["cols"], colours[a:a + step], part(opt["surface"], a),
               part(opt["depthinv"], a), opt["normals"], **c["params"])
    return vertices, triangles, colours, opt


def outputs_with_canary(lay, names):
    """flat buffers with one canary element behind the plane -> {name: (buffer, the plane's view)}"""
    H, W = lay["H"], lay["W"]
    out = {}
    for o in names:
        n = H * W * 3 if o == "atlas" else H * W
        buf = torch.full((n + (3 if o == "atlas" else 1),), CANARY[o], dtype=torch.uint8 if o == "atlas" else torch.int32, device="cuda")
        out[o] = (buf, buf[:n].view((H, W, 3) if o == "atlas" else (H, W)))
    return out


def assert_finished(tx, c, exp, mode, colours_in=None, names=OUTPUTS, triangles=None):
    """one finish and one uv into outputs with a canary behind them: the requested outputs' bytes, the canaries, the counts per view"""
    names = [o for o in names if o != "best_view" or mode == "best"]
    lay, n_t = tx.layout, tx.n_triangles
    cin = None if colours_in is None else dev(colours_in)
    tri = dev(c["triangles"]) if triangles is None else triangles
    out = outputs_with_canary(lay, names)
    uv = torch.full((n_t * 6 + 1,), UV_CANARY, dtype=torch.float32, device="cuda")
    tx.ctx.wait_torch_stream()
    tx.finish_into(tri if cin is not None else None, cin, **{o: out[o][1] for o in names})
    tx.uv_into(uv[:n_t * 6].view(n_t, 3, 2))
    tx.ctx.sync()
    for o in names:
        got = out[o][1].cpu().numpy()
        want = exp[o].view(np.int32) if exp[o].dtype == U32 else exp[o]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (o, np.argwhere(got != want)[:5])
        assert (out[o][0][out[o][1].numel():] == CANARY[o]).all(), o
    assert uv[:n_t * 6].cpu().numpy().tobytes() == exp["uv"].tobytes() and float(uv[-1]) == UV_CANARY
    if len(exp["counts"]):
        got = np.array([[k[x] for x in CM.COUNTS] for k in tx.counts()], np.int64)
        assert (got == exp["counts"]).all(), (got, exp["counts"])


def assert_textured(tx, c, mode, split=None, colours_in=None, drop=(), names=OUTPUTS, exp=None):
    exp = mirror(c, mode, colours_in=colours_in, drop=drop) if exp is None else exp
    lay = tx.begin(len(c["triangles"]), c["patch"], c["tiles_x"], mode)
    assert exp["atlas"].shape == (lay["H"], lay["W"], 3)
    held = add_views(tx, c, split, drop)
    assert_finished(tx, c, exp, mode, colours_in, names, held[1])
    del held
    return exp


def some_colours(n, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(U8)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
N_V = 40


@functools.lru_cache(maxsize=None)
def size_case(n_t, n, tiles_x, V):
    c = random_mesh_case(N_V, n_t, V, n, tiles_x, seed=n_t + 7 * n + V)
    return c, {mode: mirror(c, mode, colours_in=some_colours(N_V)) for mode in ("mean", "best")}


@pytest.mark.parametrize("n", [2, 3, 6, 14])
@pytest.mark.parametrize("n_t", [0, 1, 2, 3, 5, 129])
def test_sizes_tiles_and_chunks(tx, n_t, n):
    """T^2 = 16, 25, 64, 256: a tile below, astride, equal to and above a wave; tiles_x = 1, the default and 4, which leaves the last row
    of tiles partly empty for every n_t here; 1, 16, 17 and 33 views: one launch, a full chunk, a chunk and one view, three launches"""
    widths = (1, TX.layout(n_t, n)["tiles_x"], 4)
    assert ((n_t + 1) // 2) % 4 != 0 or n_t == 0
    for k, V in enumerate((1, 16, 17, 33)):
        for tiles_x in (widths[k % 3], widths[(k + 1) % 3]):
            c, exp = size_case(n_t, n, tiles_x, V)
            for mode in ("mean", "best"):
                assert_textured(tx, c, mode, colours_in=some_colours(N_V), exp=exp[mode])


# ---- the CPU file's cases ----------------------------------------------------------------------------------------------------------------------
def test_hand_and_boundary_cases(tx):
    img = np.zeros((1, 2, 2, 3), U8)
    beside = mesh_case([(50, 50, 1), (60, 50, 1), (50, 60, 1)], [(0, 1, 2)], img, patch=3)
    for mode in ("mean", "best"):
        exp = assert_textured(tx, hand_case(), mode)
        assert all(exp["atlas"][j, i].tolist() == b for (i, j), b in HAND_BYTES.items())
        for corner in ((0, 255, 255), (255, 0, 0), (3, 4, 8)):                 # the fallback's rounding and both clamps on the gutter
            cin = np.repeat(np.array(corner, U8)[:, None], 3, 1)
            exp = assert_textured(tx, beside, mode, colours_in=cin)
            assert exp["atlas"][2, 1, 0] == {0: 255, 255: 0, 3: 9}[corner[0]] and exp["atlas"][0, 1, 0] == {0: 128, 255: 128, 3: 4}[corner[0]]
        assert_textured(tx, beside, mode)
        for bad in (np.nan, np.inf, -np.inf):                                   # a non-finite corner gates every texel of its triangle
            for corner in range(3):
                for n in (2, 3, 6):
                    v = np.array([(1, 1, 1), (6, 1, 1), (1, 6, 1), (6, 6, 1), (1, 6, 1), (6, 1, 1)], F)
                    v[corner, 1] = bad
                    exp = assert_textured(tx, mesh_case(v, [(0, 1, 2), (3, 4, 5)], np.full((1, 8, 8, 3), 77, U8), patch=n), mode, colours_in=some_colours(6))
                    assert exp["counts"][0, 0] == exp["counts"][0, 5] == TX.layout(2, n)["texels_per_triangle"]
        rng = np.random.default_rng(8)                                          # a shared edge
        shared = mesh_case([(3.3, 2.1, 1), (27.9, 4.7, 1), (14.2, 21.6, 1), (17.1, -9.5, 1.0)], [(0, 1, 2), (0, 1, 3)], rng.integers(0, 256, (2, 24, 32, 3)).astype(U8),
                           normals=rng.normal(size=(4, 3)) * 0.2 + (0, 0, -1), patch=5, t=np.array([[0, 0, 0], [0.1, 0, 0]]), min_cos=0.0)
        assert_textured(tx, shared, mode)
        for n in (2, 6, 14):                                                    # the ramp
            exp = assert_textured(tx, mesh_case(QUAD, [(0, 1, 2), (0, 2, 3)], ramp_image(1.37, 0.61), patch=n), mode)
            assert exp["counts"][0, 5] == 2 * TX.layout(2, n)["texels_per_triangle"]


def test_every_combination_of_inputs(tx):
    c = random_mesh_case(N_V, 37, 17, 6, 3, seed=41)
    cin = some_colours(N_V, 9)
    for k in range(len(OPTIONAL) + 1):
        for drop in itertools.combinations(OPTIONAL, k):
            for mode in ("mean", "best"):
                for colours_in in (None, cin):
                    assert_textured(tx, c, mode, colours_in=colours_in, drop=drop)


def test_each_output_absent_in_turn(tx):
    c = random_mesh_case(N_V, 45, 5, 3, 4, seed=43)
    cin = some_colours(N_V, 11)
    for mode in ("mean", "best"):
        exp = mirror(c, mode, colours_in=cin)
        used = exp["views_used"]
        assert (used == 0).any() and (used > 0).any()
        for k in (1, 2, 3):
            for names in itertools.combinations(OUTPUTS, k):
                assert_textured(tx, c, mode, colours_in=cin, names=names, exp=exp)
        out = tx.finish(dev(c["triangles"]), dev(cin))        # the same state once more, through the call that allocates
        assert sorted(out) == sorted(o for o in OUTPUTS if o != "best_view" or mode == "best")
        assert all(out[o].cpu().numpy().tobytes() == exp[o].tobytes() for o in out)
        assert tx.uv().cpu().numpy().tobytes() == exp["uv"].tobytes()
        tx.finish_into()                                      # no output at all: nothing is launched
        tx.ctx.sync()


# ---- call order ----------------------------------------------------------------------------------------------------------------------------
def test_calls_in_every_order_on_exact_capacity(ctx):
    big, small = random_mesh_case(N_V, 129, 17, 6, 4, seed=5), random_mesh_case(25, 30, 3, 14, 1, rows=9, cols=11, seed=6)
    slots = max(TX.layout(129, 6, 4)["slots"], TX.layout(30, 14, 1)["slots"])
    assert slots == 65 * 64 > TX.layout(30, 14, 1)["slots"] == 15 * 256
    h = TX.Texturer(ctx, 129, slots)
    views = lambda c, a, b: dict(c, R=c["R"][a:b], t=c["t"][a:b], colours=c["colours"][a:b], surface=c["surface"][a:b], depthinv=c["depthinv"][a:b])
    try:
        for mode in ("mean", "best"):
            whole, first = mirror(big, mode), mirror(views(big, 0, 16), mode)
            h.begin(129, 6, 4, mode)
            held = [add_views(h, views(big, 0, 16))]
            assert_finished(h, big, first, mode)
            assert_finished(h, big, first, mode)                # finish changes nothing
            held.append(add_views(h, views(big, 16, 17)))
            assert_finished(h, big, whole, mode)                # views may follow a finish: the 17th has the global index 16
            assert h.counts(16, 1) == [dict(zip(CM.COUNTS, whole["counts"][16].tolist()))]
            for split in (1, 16):
                assert_textured(h, big, mode, split=split, exp=whole)
            assert_textured(h, small, mode)                     # a second begin with another n_t, patch and image size
            assert_textured(h, big, mode, exp=whole)
            del held
        with pytest.raises(ValueError):
            h.begin(130, 6, 4)
        with pytest.raises(ValueError):
            h.begin(129, 7, 4)                                  # more slots than the handle has
        with pytest.raises(ValueError):
            add_views(h, random_mesh_case(N_V, 128, 1, 6, 4, seed=1))
        assert_textured(h, big, "mean")
    finally:
        h.close()


# ---- a mixed scene ---------------------------------------------------------------------------------------------------------------------------
def grid_quad(nx, ny, x0, x1, y0, y1, z):
    """(nx x ny vertices over the rectangle at depth z(x, y), their triangles)"""
    gx, gy = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
    v = np.stack([gx, gy, z(gx, gy)], -1).reshape(-1, 3)
    cell = np.array([(j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i) for j in range(ny - 1) for i in range(nx - 1)])
    return v, np.concatenate([cell[:, [0, 1, 2]], cell[:, [0, 2, 3]]])


@functools.lru_cache(maxsize=None)
def mixed_scene():
    """a wavy 32 x 32 vertex sheet around z = 2 that reaches beside the 64 x 48 images (OUTSIDE), a small quad at z = 1.2 in front of it
    (HIDDEN), a quad behind the cameras and one beyond z_max (GATED), a fifth of the normals turned away (AVERTED), holes in the
    keyframes' inverse depth (UNMEASURED); 17 cameras near the origin: 1 930 triangles"""
    rng = np.random.default_rng(77)
    sheet, st = grid_quad(32, 32, -2.4, 2.4, -1.8, 1.8, lambda x, y: 2.0 + 0.15 * np.sin(2.1 * x) * np.cos(1.7 * y))
    front, ft = grid_quad(2, 2, -0.35, 0.3, -0.25, 0.3, lambda x, y: 1.2 + 0 * x)
    behind, bt = grid_quad(2, 2, -0.5, 0.5, -0.5, 0.5, lambda x, y: -1.0 + 0 * x)
    far, rt = grid_quad(2, 2, -0.5, 0.5, -0.5, 0.5, lambda x, y: 9.0 + 0 * x)
    parts, tris, base = [sheet, front, behind, far], [st, ft, bt, rt], 0
    for k, p in enumerate(parts):
        tris[k] = tris[k] + base
        base += len(p)
    verts, tri = np.concatenate(parts).astype(F), np.concatenate(tris).astype(U32)
    nrm = np.tile(np.array([0.0, 0.0, -1.0]), (len(verts), 1)) + rng.normal(0, 0.2, (len(verts), 3))
    nrm[rng.random(len(verts)) < 0.2] *= -1
    rows, cols, V = 48, 64, 17
    K = (0.9 * cols, 0.9 * cols, (cols - 1) / 2, (rows - 1) / 2)
    R, t = [], []
    for v in range(V):
        w = rng.normal(0, 0.08, 3)
        a = np.linalg.norm(w)
        k = w / a
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R.append(np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx)
        t.append(rng.normal(0, 0.1, 3))
    colours = rng.integers(0, 256, (V, rows, cols, 3)).astype(U8)
    return dict(vertices=verts, triangles=tri, normals=nrm.astype(F), R=np.stack(R), t=np.stack(t), K=K, rows=rows, cols=cols, colours=colours, patch=6,
                tiles_x=TX.layout(len(tri), 6)["tiles_x"],
                params=dict(z_min=0.3, z_max=6.0, surface_tolerance=0.03, measured_tolerance=0.05, min_cos=0.3, two_sided=False))


def test_mixed_scene_with_every_class(ctx, tx):
    c = dict(mixed_scene())
    n_t = len(c["triangles"])
    assert 1900 <= n_t <= 2100
    depth = RS.render_mesh(ctx, dev(c["vertices"]), dev(c["triangles"]), c["R"], c["t"], c["K"], c["rows"], c["cols"], z_min=0.3, z_max=6.0,
                           outputs=("depth",))["depth"].cpu().numpy()
    rng = np.random.default_rng(78)
    with np.errstate(all="ignore"):
        iD = (1.0 / depth).astype(F)
    iD[rng.random(iD.shape) < 0.08] = 0.0
    iD[:, 5:9, 40:50] = np.nan
    c.update(surface=depth, depthinv=iD)
    cin = some_colours(len(c["vertices"]), 13)
    for mode in ("mean", "best"):
        exp = mirror(c, mode, colours_in=cin)
        total = exp["counts"].sum(0)
        print("mixed scene:", dict(zip(CM.COUNTS, total.tolist())), "texels", n_t * 26, "textured", int((exp["views_used"] != 0).sum()))
        assert (total > 0).all() and (exp["counts"].sum(1) == n_t * 26).all()
        assert (exp["views_used"] >= 2).any() and (exp["atlas"] != 0).any()
        tx.timing(True)
        assert_textured(tx, c, mode, colours_in=cin, exp=exp)
        ms = tx.timing(False)
        print("mixed scene ms:", ms)
        assert all(v > 0 for v in ms.values())


def test_two_quads_hide_each_other(ctx, tx):
    """two 9 x 9 vertex quads over x, y in [-1, 1] at z = 2 and z = 3; view 0 looks along +z from the origin, view 1 along -z from z = 5:
    each view's nearer quad hides the other one, so every texel some view took has its own side's colour"""
    v0, t0 = grid_quad(9, 9, -1, 1, -1, 1, lambda x, y: 2.0 + 0 * x)
    v1, t1 = grid_quad(9, 9, -1, 1, -1, 1, lambda x, y: 3.0 + 0 * x)
    verts, tris = np.concatenate([v0, v1]).astype(F), np.concatenate([t0, t1 + len(v0)]).astype(U32)
    R, t = np.stack([np.eye(3), np.diag([-1.0, 1.0, -1.0])]), np.array([[0.0, 0, 0], [0, 0, 5.0]])
    K, front, back = (16.0, 16.0, 16.0, 16.0), (200, 100, 50), (20, 40, 61)
    img = np.stack([np.broadcast_to(np.array(x, U8), (33, 33, 3)) for x in (front, back)])
    depth = RS.render_mesh(ctx, dev(verts), dev(tris), R, t, K, 33, 33, outputs=("depth",))["depth"].cpu().numpy()
    c = mesh_case(verts, tris, img, K, R, t, surface=depth, patch=3, tiles_x=8, z_min=0.05, z_max=20.0, surface_tolerance=0.02)
    n_half = len(t0) * 8                                        # the texels of a quad's triangles
    col, row = TM.atlas_pixels(len(tris), 3, 8)
    for mode in ("mean", "best"):
        exp = assert_textured(tx, c, mode)
        used, rgb = exp["views_used"][row, col].reshape(-1), exp["atlas"][row, col].reshape(-1, 3)
        assert used.max() == 1 and (used[:n_half] == 1).sum() > n_half // 2 and (used[n_half:] == 1).sum() > n_half // 2
        assert (rgb[:n_half][used[:n_half] == 1] == front).all() and (rgb[n_half:][used[n_half:] == 1] == back).all()
        assert exp["counts"][:, 2].min() >= n_half // 2         # the farther quad is hidden in each view
    exp = assert_textured(tx, c, "best", drop=("surface",))
    assert exp["views_used"].max() == 2


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_host_side_refusals_leave_state_and_outputs(tx):
    c = random_mesh_case(N_V, 61, 3, 6, 4, rows=20, cols=30, seed=9)
    n_t, n_v, p0 = 61, N_V, c["params"]
    L = tx.L
    nan, inf = float("nan"), float("inf")
    bad_tri = c["triangles"].copy(); bad_tri[37, 1] = n_v
    for mode in ("mean", "best"):
        exp = mirror(c, mode)
        lay = tx.begin(n_t, 6, 4, mode)
        v, tri, colours, opt = add_views(tx, c)
        out = outputs_with_canary(lay, OUTPUTS)
        uv = torch.full((n_t * 6 + 2,), UV_CANARY, dtype=torch.float32, device="cuda")
        bad = dev(bad_tri)
        p = {k: x.data_ptr() for k, x in dict(v=v, tri=tri, bad=bad, nr=opt["normals"], col=colours, sf=opt["surface"], iD=opt["depthinv"], uv=uv,
                                              **{o: out[o][0] for o in out}).items()}

        def view(R=np.eye(3), t=(0, 0, 0), col=p["col"], sf=p["sf"], iD=p["iD"]):
            return RC.View(RC.Pose((C.c_double * 9)(*np.asarray(R, np.float64).reshape(9)), (C.c_double * 3)(*t)), col, sf, iD)

        def add(h=tx._h, v=p["v"], nr=p["nr"], nv=n_v, tri=p["tri"], nt=n_t, V=1, views=view(), K=c["K"], rows=20, cols=30, params=True, **kw):
            prm = RC.Params(*[kw.get(k, p0[k]) for k in ("z_min", "z_max", "surface_tolerance", "measured_tolerance", "min_cos")], kw.get("two_sided", 0))
            return L.rgbid_texture_add(h, v, nr, nv, tri, nt, V, C.byref(views) if views is not None else None, (C.c_float * 4)(*K) if K is not None else None,
                                       rows, cols, C.byref(prm) if params else None)

        tx.ctx.wait_torch_stream()
        refusals = [dict(h=None), dict(views=None), dict(K=None), dict(params=False), dict(V=0), dict(V=-1), dict(V=RC.MAX_VIEWS - 2), dict(nt=n_t - 1),
                    dict(nt=n_t + 1), dict(nt=CAP_T + 1), dict(rows=0), dict(cols=0), dict(rows=RC.MAX_DIM + 1), dict(cols=RC.MAX_DIM + 1),
                    dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=nan), dict(z_max=inf), dict(z_min=3.0, z_max=2.0),
                    dict(surface_tolerance=-1e-9), dict(surface_tolerance=nan), dict(surface_tolerance=inf), dict(measured_tolerance=-1.0),
                    dict(measured_tolerance=nan), dict(measured_tolerance=inf), dict(min_cos=-1e-6), dict(min_cos=1.0001), dict(min_cos=nan),
                    dict(two_sided=2), dict(two_sided=-1),
                    dict(K=(nan, 1, 0, 0)), dict(K=(1, inf, 0, 0)), dict(K=(0, 1, 0, 0)), dict(K=(1, 0, 0, 0)), dict(K=(1, 1, nan, 0)), dict(K=(1, 1, 0, inf)),
                    dict(views=view(t=(nan, 0, 0))), dict(views=view(R=np.full((3, 3), inf))), dict(views=view(R=np.full((3, 3), 1e300))),
                    dict(views=view(t=(1e300, 0, 0))), dict(views=view(col=None)), dict(views=view(sf=p["sf"] + 2)), dict(views=view(iD=p["iD"] + 1)),
                    dict(v=None), dict(v=p["v"] + 2), dict(nr=p["nr"] + 1),
                    dict(tri=None), dict(tri=p["tri"] + 2), dict(nv=0), dict(nv=(1 << 31) + 1), dict(tri=p["bad"]), dict(nv=int(c["triangles"].max()))]
        for kw in refusals:
            assert add(**kw) == -1, kw
        fin = lambda h=tx._h, tri=None, cin=None, nv=0, atlas=p["atlas"], used=p["views_used"], best=p["best_view"] if mode == "best" else None: \
            L.rgbid_texture_finish(h, tri, cin, nv, atlas, used, best)
        bad_finish = [dict(h=None), dict(used=p["views_used"] + 2), dict(best=p["best_view"] + 1), dict(cin=p["col"]), dict(cin=p["col"], tri=p["tri"] + 2, nv=n_v),
                      dict(cin=p["col"], tri=p["tri"], nv=0), dict(cin=p["col"], tri=p["tri"], nv=(1 << 31) + 1)] + ([dict(best=p["best_view"])] if mode == "mean" else [])
        for kw in bad_finish:
            assert fin(**kw) == -1, kw
        assert L.rgbid_texture_uv(None, p["uv"]) == -1 and L.rgbid_texture_uv(tx._h, None) == -1 and L.rgbid_texture_uv(tx._h, p["uv"] + 2) == -1
        for args in ((CAP_T + 1, 6, 4, 0), (n_t, 6, 4, 2), (n_t, 6, 4, -1), (n_t, 1, 4, 0), (n_t, 31, 4, 0), (n_t, 6, 0, 0), (n_t, 6, 2049, 0), (CAP_T, 30, 64, 0)):
            assert L.rgbid_texture_begin(tx._h, *args) == -1, args
        cnt = (C.c_ulonglong * 24)()
        for first, V, o in ((0, 4, cnt), (-1, 1, cnt), (3, 1, cnt), (0, 0, cnt), (0, 3, None), (2, 2, cnt)):
            assert L.rgbid_texture_counts(tx._h, first, V, o) == -1, (first, V)
        tx.ctx.sync()
        assert all((out[o][0] == CANARY[o]).all() for o in out) and (uv == UV_CANARY).all()
        assert tx.views == 3 and L.rgbid_texture_counts(tx._h, 0, 3, cnt) == 0 and list(cnt[:18]) == exp["counts"].reshape(-1).tolist()
        assert_finished(tx, c, exp, mode)                     # the state is what the three views left
    fresh = TX.Texturer(tx.ctx, 10, 1000)
    try:
        assert L.rgbid_texture_finish(fresh._h, None, None, 0, None, None, None) == -1 and L.rgbid_texture_counts(fresh._h, 0, 1, cnt) == -1      # no begin
        assert L.rgbid_texture_uv(fresh._h, p["uv"]) == -1
        prm = RC.Params(0.5, 4.0, 0.1, 0.1, 0.2, 0)
        assert L.rgbid_texture_add(fresh._h, p["v"], None, n_v, p["tri"], 10, 1, C.byref(view()), (C.c_float * 4)(*c["K"]), 20, 30, C.byref(prm)) == -1
        for f in (lambda: fresh.add(v, tri, c["R"], c["t"], c["K"], 20, 30, colours), fresh.finish, fresh.finish_into, fresh.uv):
            with pytest.raises(ValueError):
                f()
    finally:
        fresh.close()
    for cap in ((0, 10), ((1 << 31), 10), (10, 0), (10, (1 << 28) + 1), (2.0, 10)):
        with pytest.raises(ValueError):
            TX.Texturer(tx.ctx, *cap)
    tx.begin(n_t, 6, 4, "mean")
    v, tri, colours = dev(c["vertices"]), dev(c["triangles"]), dev(c["colours"])
    good = dict(R=c["R"], t=c["t"], K=c["K"], rows=20, cols=30, colours=colours)
    for kw in (dict(rows=21), dict(colours=colours[:2]), dict(surface=dev(c["surface"])[:, :19]), dict(depthinv=dev(c["depthinv"]).double()),
               dict(normals=dev(c["normals"])[:-1]), dict(z_min=0), dict(min_cos=2), dict(surface_tolerance=-1), dict(two_sided="no"), dict(K=(0, 1, 0, 0))):
        with pytest.raises(ValueError):                     # the Python checks come first
            tx.add(v, tri, **dict(good, **kw))
    for mesh in ((v, tri[:-1]), (v, tri.float()), (v.double(), tri), (v[:0], tri)):
        with pytest.raises(ValueError):
            tx.add(*mesh, **good)
    with pytest.raises(RuntimeError):                       # the index beyond the vertices is the library's to find
        tx.add(v, dev(bad_tri), **good)
    with pytest.raises(ValueError):
        tx.finish_into(best_view=torch.zeros((tx.layout["H"], tx.layout["W"]), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        tx.finish_into(colours_in=dev(some_colours(n_v)))
    with pytest.raises(ValueError):
        tx.finish_into(atlas=torch.zeros((tx.layout["H"], tx.layout["W"] + 1, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        tx.counts()
    assert tx.views == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_texture_mesh_against_the_mirror(ctx):
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
    v, col, tri, nrm = TS.fuse(ctx, kfs, K_SMALL, rows, cols, bounds=[*(lo - 0.2), *(hi + 0.2)], voxel=voxel, normals=True, simplify=4 * voxel)[:4]
    n_t = tri.shape[0]
    assert 200 < n_t < 20000
    R, tw = np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs])
    depth = RS.render_mesh(ctx, v, tri, R, tw, K_SMALL, rows, cols, outputs=("depth",))["depth"].cpu().numpy()
    for mode, measured in (("mean", None), ("best", 0.1)):
        timing = {}
        got = TX.texture_mesh(ctx, v, tri, kfs, K_SMALL, rows, cols, patch=6, normals=nrm, colours=col, mode=mode, surface_tolerance=2 * voxel,
                              measured_tolerance=measured, batch=3, timing=timing)
        lay = got["layout"]
        exp = TM.texture_numpy(v.cpu().numpy(), tri.cpu().numpy(), R, tw, K_SMALL, rows, cols, [k["colour"].cpu().numpy() for k in kfs], 6, lay["tiles_x"],
                               mode, col.cpu().numpy(), surface=depth, depthinv=None if measured is None else [k["depthinv"].cpu().numpy() for k in kfs],
                               normals=nrm.cpu().numpy(), z_min=0.05, z_max=20.0, surface_tolerance=2 * voxel, measured_tolerance=measured or 0.0, min_cos=0.2,
                               two_sided=False)
        assert lay == TX.layout(n_t, 6) and got["atlas"].cpu().numpy().tobytes() == exp["atlas"].tobytes()
        assert got["views_used"].cpu().numpy().tobytes() == exp["views_used"].tobytes() and got["uv"].cpu().numpy().tobytes() == exp["uv"].tobytes()
        assert [[k[x] for x in CM.COUNTS] for k in got["counts"]] == exp["counts"].tolist()
        textured = int((exp["views_used"] != 0).sum())
        print("texture_mesh:", mode, dict(triangles=n_t, texels=got["texels"], textured=got["textured"], fallback=got["fallback"]), timing)
        assert got["texels"] == n_t * 26 and got["textured"] == textured > got["texels"] // 2 and got["fallback"] == got["texels"] - textured
        assert sorted(timing) == ["accumulate", "raster", "resolve"] and all(x > 0 for x in timing.values())
    with pytest.raises(ValueError):
        TX.texture_mesh(ctx, v, tri, [dict(k, colour=None) for k in kfs], K_SMALL, rows, cols)
    with pytest.raises(ValueError):
        TX.texture_mesh(ctx, v, tri, kfs, K_SMALL, rows, cols, patch=31)


def test_track_dataset_mesh_texture(ctx, tmp_path):
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("tex", ["--mesh-texture", str(tmp_path / "tex.obj"), "--mesh-texture-patch", "4", "--mesh-texture-mode", "best",
                                                "--mesh-texture-tolerance", "0.08"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply"), "--mesh-voxel", "0.05", "--mesh-normals",
                                   "--mesh-simplify", "0.15"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = [l.replace("tex.ply", "plain.ply").replace("traj_tex", "traj_plain") for l in r.stdout.splitlines() if "frames/s" not in l]
    added = [l for l in said["tex"] if "mesh texture (best)" in l]
    assert len(added) == 1 and [l for l in said["tex"] if l not in added] == said["plain"]      # without the options: today's lines
    a, b = ((tmp_path / f"{x}.ply").read_bytes() for x in ("plain", "tex"))
    assert a == b and (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_tex.txt").read_bytes()
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("tex.")) == ["tex.mtl", "tex.obj", "tex.ply", "tex.png"]
    verts, _, tris, nrm = TS.read_mesh_ply(a)
    obj = TX.read_obj(str(tmp_path / "tex.obj"))
    lay = TX.layout(len(tris), 4)
    assert obj["vertices"].tobytes() == verts.tobytes() and obj["triangles"].tobytes() == np.asarray(tris).astype(U32).tobytes()
    assert obj["normals"].tobytes() == nrm.tobytes() and obj["uv"].tobytes() == TM.uv_of(len(tris), 4, lay["tiles_x"]).tobytes()
    assert obj["atlas"].shape == (lay["H"], lay["W"], 3) and obj["texture"] == "tex.png" and obj["atlas"].any()
    words = added[0].split()
    textured, texels = int(words[words.index("of") - 1]), int(words[words.index("of") + 1])
    assert texels == len(tris) * lay["texels_per_triangle"] and 0 < textured <= texels and f"atlas {lay['W']} x {lay['H']}" in added[0]
    assert all(f" {k}" in added[0] for k in CM.COUNTS) and added[0].endswith("tex.obj")
