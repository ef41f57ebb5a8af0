"""GPU tests of the denoising stage (include/rgbid_denoise.h, csrc/kernels_denoise.hip, rgbid.denoise): the four counts, the face table,
the filtered normals and the positions byte for byte against the numpy restatement (tests/denoise_mirror.py) on the meshes of
tests/test_cpu_denoise.py, at 0, 1, 2 and 7 iterations of each kind (both parities of both ping-pongs) and thresholds 0, 0.4 and 0.9,
canaries behind every output; triangle and vertex counts either side of the block, of the tiles of the sort and the scan and of a change in
the sort's pass count; 100 000 triangles over 600 000 vertices; a hub row of 1 024; a row with repeats; plans, normals and vertices calls in
every order on one handle of exact capacities; every refusal; and the options of rgbid.tsdf and tools/track_dataset.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import denoise as DN, sequence, synth, tsdf as TS, tum
from tests import denoise_mirror as DM
from tests import smooth_mirror as SM
from tests import tsdf_mirror as TM
from tests.test_cpu_denoise import all_cases, centroid_mesh, denoised, normals_of, table_of
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

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
def dn(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh of another size"""
    h = DN.Denoiser(ctx, CAP_V, CAP_T)
    yield h
    h.close()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def raw(x):
    return x.cpu().numpy().tobytes()


def full(rows, cols, dtype, value):
    return torch.full((rows + PAD,) + cols, value, dtype=dtype, device="cuda")


def assert_planned(dn, tri, tab):
    """the plan's counts, and the face table in buffers with PAD canary rows behind them"""
    got = dn.plan(tri, tab["n_v"])
    assert got == tab["counts"], (got, tab["counts"])
    n_v, n_f = tab["n_v"], len(tab["faces"])
    off, fc = full(n_v + 1, (), torch.int32, -5), full(n_f, (), torch.int32, -6)
    dn.ctx.wait_torch_stream()
    dn.faces_into(off, fc)
    dn.ctx.sync()
    assert raw(off[:n_v + 1]) == tab["offsets"].tobytes() and (off[n_v + 1:] == -5).all()
    assert raw(fc[:n_f]) == tab["faces"].tobytes() and (fc[n_f:] == -6).all()


def assert_normals(dn, vdev, exp, iterations, threshold):
    """one normals call into a buffer with PAD canary rows: the normals' bytes, the canary, the input untouched"""
    n_t = len(exp)
    before = raw(vdev)
    out = full(n_t, (3,), torch.float32, 7.0)
    dn.ctx.wait_torch_stream()
    dn.normals_into(vdev, out[:n_t], iterations, threshold)
    dn.ctx.sync()
    got = out[:n_t].cpu().numpy()
    assert got.tobytes() == exp.tobytes(), (iterations, threshold, np.nonzero((got.view(U32) != exp.view(U32)).any(1))[0][:10])
    assert (out[n_t:] == 7.0).all() and raw(vdev) == before


def assert_vertices(dn, vdev, ndev, exp, iterations):
    n_v = len(exp)
    before = raw(vdev), raw(ndev)
    out = full(n_v, (3,), torch.float32, -3.0)
    dn.ctx.wait_torch_stream()
    dn.vertices_into(vdev, ndev, out[:n_v], iterations)
    dn.ctx.sync()
    got = out[:n_v].cpu().numpy()
    assert got.tobytes() == exp.tobytes(), (iterations, np.nonzero((got.view(U32) != exp.view(U32)).any(1))[0][:10])
    assert (out[n_v:] == -3.0).all() and (raw(vdev), raw(ndev)) == before


def assert_denoised(dn, m, normal_iterations=(2,), vertex_iterations=(2,), thresholds=(0.4,)):
    """a mesh that is no case of the CPU file: plan, normals and vertices against the mirror -> the face table"""
    v = np.ascontiguousarray(m["vertices"], F)
    tab = DM.face_table(m["triangles"], len(v))
    vdev = dev(v)
    assert_planned(dn, dev(m["triangles"]), tab)
    for T in thresholds:
        for n in normal_iterations:
            nrm = DM.normals(v, tab, n, T)
            assert_normals(dn, vdev, nrm, n, T)
    for k in vertex_iterations:
        assert_vertices(dn, vdev, dev(nrm), DM.vertices(v, nrm, tab, k), k)
    return tab


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_cases_against_the_mirror(dn, name):
    """0, 1, 2 and 7 iterations of each kind: both parities of both ping-pongs; the thresholds 0, 0.4 and 0.9"""
    m, tab = all_cases()[name], table_of(name)
    tri, vdev = dev(m["triangles"]), dev(m["vertices"])
    assert_planned(dn, tri, tab)
    for T in (0.0, 0.4, 0.9):
        for n in (0, 1, 2, 7):
            assert_normals(dn, vdev, normals_of(name, n, T), n, T)
    ndev = dev(normals_of(name, 2, 0.4))
    for k in (0, 1, 2, 7):
        assert_vertices(dn, vdev, ndev, denoised(name, 2, k, 0.4), k)
    pos, nrm = dn.run(vdev, 2, 7, 0.4)                           # the allocating forms
    assert raw(pos) == denoised(name, 2, 7, 0.4).tobytes() and raw(nrm) == normals_of(name, 2, 0.4).tobytes()
    got = dn.faces()
    assert raw(got["offsets"]) == tab["offsets"].tobytes() and raw(got["faces"]) == tab["faces"].tobytes()


def test_vertex_pass_sums_in_ascending_triangle_order(dn):
    """the supplied normals of tests/test_cpu_denoise.py: 1 + X - X is 0 in ascending order; normals that are not unit or not finite"""
    v = np.array([(0, 0, 0), (1, 0, 1.5), (0, 1, 1.5), (1, 0, 1.5e30), (0, 1, 1.5e30), (1, 0, -1.5e30), (0, 1, -1.5e30)], F)
    tri = np.array([(0, 1, 2), (0, 3, 4), (0, 5, 6)], U32)
    tab = DM.face_table(tri, 7)
    assert_planned(dn, dev(tri), tab)
    for nrm in (np.tile(np.array([0, 0, 1], F), (3, 1)), np.array([(0, 0, 2), (np.nan, 0, 1), (0, 0, 0)], F)):
        exp = DM.vertex_pass(v, nrm, tab)
        assert exp[0].tolist() in ([0, 0, 0], [0, 0, 4])
        assert_vertices(dn, dev(v), dev(nrm), exp, 1)
    back = DM.face_table(tri[::-1].copy(), 7)
    assert_planned(dn, dev(tri[::-1].copy()), back)
    exp = DM.vertex_pass(v, np.tile(np.array([0, 0, 1], F), (3, 1)), back)
    assert exp[0].tolist() == [0, 0, F(1 / 3)]
    assert_vertices(dn, dev(v), dev(np.tile(np.array([0, 0, 1], F), (3, 1))), exp, 1)


def test_centroid_adds_the_corners_in_order(dn):
    """((X - X) + 1.5) / 3 is 0.5 and (X + (-X + 1.5)) / 3 is 0: the corner at 1.5 moves to 0.5"""
    m = centroid_mesh()
    tab = DM.face_table(m["triangles"], 3)
    nrm = np.array([(0, 0, 1)], F)
    exp = DM.vertex_pass(m["vertices"], nrm, tab)
    assert exp[2].tolist() == [0, 1, 0.5]
    assert_planned(dn, dev(m["triangles"]), tab)
    assert_vertices(dn, dev(m["vertices"]), dev(nrm), exp, 1)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
def random_mesh(n_t, n_v, seed, top=0):
    """n_t random triangles over n_v vertices at random positions, the first `top` of them among the 40 largest indices, the last one
    naming the last vertex; some vertices not finite"""
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, n_v, (n_t, 3)).astype(U32)
    tri[:top] = rng.integers(max(n_v - 40, 0), n_v, (top, 3))
    tri[-1] = (n_v - 1, 0, max(n_v - 2, 0))
    v = rng.uniform(-1, 1, (n_v, 3)).astype(F)
    v[5::97, 1] = np.nan
    return dict(vertices=v, triangles=tri)


def strip_mesh(k, n_v, seed):
    """a strip of k triangles over the first k + 2 of n_v vertices, shuffled, as a noisy sheet: the normals hear each other"""
    rng = np.random.default_rng(seed)
    tri = (np.arange(k)[:, None] + np.arange(3)[None, :]).astype(U32)
    tri[1::2] = tri[1::2, ::-1]                                 # one orientation along the strip
    v = np.stack([np.arange(n_v) // 2, np.arange(n_v) % 2, np.zeros(n_v)], 1) + rng.normal(0, 0.05, (n_v, 3))
    return dict(vertices=v.astype(F), triangles=tri[rng.permutation(k)])


@pytest.mark.parametrize("n_t", [255, 256, 257, 341, 342, 682, 683, 1365, 1366])
def test_triangle_counts_either_side_of_a_block_and_a_tile(dn, n_t):
    """n_t = 255 - 257: the block of the passes; 3 n_t = 1023 | 1026, 2046 | 2049 and 4095 | 4098: the scan's and the sort's tiles"""
    assert 3 * 682 < RUN_TILE <= 3 * 683 and 3 * 1365 < SORT_TILE <= 3 * 1366
    tab = assert_denoised(dn, strip_mesh(n_t, n_t + 10, n_t))
    assert tab["counts"]["empty_rows"] == 8 and tab["counts"]["longest_row"] == 3 and len(tab["faces"]) == 3 * n_t
    assert_denoised(dn, random_mesh(n_t, 500, n_t))


@pytest.mark.parametrize("n_v", [255, 256, 257, 2047, 2048, 2049, 65535, 65536, 65537])
def test_vertex_counts_either_side_of_a_block_a_tile_and_a_sort_pass(dn, n_v):
    """the sort's key n_v has 8, 9, 11, 12, 16 and 17 bits: one, two and three passes; n_v + 1 offsets either side of the block and a tile"""
    tab = assert_denoised(dn, random_mesh(6000, n_v, n_v, top=3000))
    assert int(tab["triangles"].max()) == n_v - 1 and tab["counts"]["repeating_triangles"] > 100
    if n_v <= 2049:
        assert_denoised(dn, strip_mesh(n_v - 2, n_v, n_v))       # every vertex has a row


def test_many_vertices_without_a_triangle(dn):
    """100 000 random triangles over 600 000 vertices: mostly empty rows, 74 tiles of the sort"""
    m = random_mesh(100000, 600000, 1)
    m["triangles"][::50] = np.random.default_rng(2).integers(0, 40, (2000, 3))      # duplicates, repeats and long rows among the first vertices
    tab = assert_denoised(dn, m)
    c = tab["counts"]
    assert c["empty_rows"] > 300000 and c["longest_row"] > 100 and c["repeating_triangles"] > 100 and c["work"] > 300000


def test_a_hub_row_of_1024(dn):
    """every face of the fan merges the hub's row of 1 024 with two rows of one: the merge, the gather of four and its tail"""
    tab = table_of("fan")
    assert tab["counts"] == dict(empty_rows=0, longest_row=1024, repeating_triangles=0, work=1024 * 1026)
    t, _ = DM.neighbourhoods(tab)
    assert (np.bincount(t) == 1024).all()
    tab = table_of("hub_repeats")
    assert tab["counts"]["longest_row"] == 57 and tab["counts"]["repeating_triangles"] == 19


# ---- life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_calls_in_every_order_on_one_handle(ctx):
    """a handle of exactly the largest mesh's sizes: larger, smaller and empty meshes in turn; vertices before normals, normals twice,
    vertices twice on one plan; the stage timing"""
    cases = all_cases()
    names = ("random", "hand", "no_vertices", "noisy_cube", "no_triangles", "fan", "hand", "open_cube", "random")
    cap_v, cap_t = (max(len(cases[n][k]) for n in names) for k in ("vertices", "triangles"))
    h = DN.Denoiser(ctx, cap_v, cap_t)
    try:
        for i, name in enumerate(names):
            m, tab = cases[name], table_of(name)
            tri, vdev = dev(m["triangles"]), dev(m["vertices"])
            ndev = dev(normals_of(name, 2, 0.4))
            assert_planned(h, tri, tab)
            if i % 2:
                assert_vertices(h, vdev, ndev, denoised(name, 2, 1, 0.4), 1)
            assert_normals(h, vdev, normals_of(name, 2, 0.4), 2, 0.4)
            assert_vertices(h, vdev, ndev, denoised(name, 2, 2, 0.4), 2)
            assert_normals(h, vdev, normals_of(name, 1, 0.9), 1, 0.9)
            assert_vertices(h, vdev, ndev, denoised(name, 2, 7, 0.4), 7)
        with pytest.raises(ValueError):
            h.plan(tri, cap_v + 1)                               # above the capacity
        h.timing(True)
        assert_planned(h, tri, tab)
        assert_normals(h, vdev, normals_of("random", 2, 0.4), 2, 0.4)
        assert_vertices(h, vdev, ndev, denoised("random", 2, 2, 0.4), 2)
        ms = h.timing(False)
        print("denoise stage ms:", ms)
        assert tuple(ms) == DN.STAGES and all(np.isfinite(x) and x > 0 for x in ms.values())
    finally:
        h.close()


def test_refusals_and_reuse(dn):
    L = dn.L
    m, tab = all_cases()["noisy_cube"], table_of("noisy_cube")
    tri, vdev = dev(m["triangles"]), dev(m["vertices"])
    n_v, n_t = len(m["vertices"]), len(m["triangles"])
    nexp = normals_of("noisy_cube", 2, 0.4)
    ndev = dev(nexp)
    counts = (C.c_ulonglong * 4)()

    def still_works():
        assert_planned(dn, tri, tab)
        assert_normals(dn, vdev, nexp, 2, 0.4)
        assert_vertices(dn, vdev, ndev, denoised("noisy_cube", 2, 2, 0.4), 2)

    out = torch.zeros((max(n_v, n_t) + 1, 3), dtype=torch.float32, device="cuda")
    buf = torch.zeros(3 * n_t + n_v + 2, dtype=torch.int32, device="cuda")
    pv, pt, pn, po, pb = vdev.data_ptr(), tri.data_ptr(), ndev.data_ptr(), out.data_ptr(), buf.data_ptr()
    plan = lambda nv=n_v, nt=n_t, t=pt: L.rgbid_denoise_plan(dn._h, nv, nt, t, counts)
    normals = lambda i=pv, o=po, n=2, T=0.4: L.rgbid_denoise_normals(dn._h, i, o, n, T)
    vertices = lambda i=pv, nr=pn, o=po, n=2: L.rgbid_denoise_vertices(dn._h, i, nr, o, n)
    faces = lambda off=pb, fc=None: L.rgbid_denoise_faces(dn._h, off, fc)
    still_works()
    # a triangle that names a vertex that does not exist: the plan is refused, the former one is gone, the next one is right
    for where in (0, n_t // 2, n_t - 1):
        for value in (n_v, 0xFFFFFFFF):
            bad = np.array(m["triangles"], U32)
            bad[where, where % 3] = value
            with pytest.raises(Exception, match="rgbid error -1"):
                dn.plan(dev(bad), n_v)
            assert normals() == -1 and vertices() == -1 and faces() == -1
        still_works()
    # the host-side refusals keep the plan: the calls after them are the former plan's
    for r in (lambda: plan(nv=CAP_V + 1), lambda: plan(nt=CAP_T + 1), lambda: plan(t=None), lambda: plan(t=pt + 1), lambda: plan(t=pt + 2),
              lambda: plan(nv=0)):
        dn.ctx.wait_torch_stream()
        assert r() == -1
        assert_normals(dn, vdev, normals_of("noisy_cube", 1, 0.4), 1, 0.4)
        assert_vertices(dn, vdev, ndev, denoised("noisy_cube", 2, 1, 0.4), 1)
    inf, nan = float("inf"), float("nan")
    for r in (lambda: normals(i=None), lambda: normals(o=None), lambda: normals(i=pv + 2), lambda: normals(o=po + 1), lambda: normals(o=pv),
              lambda: normals(i=po), lambda: normals(i=po + 12), lambda: normals(n=257), lambda: normals(n=0xFFFFFFFF), lambda: normals(T=-0.1),
              lambda: normals(T=1.0), lambda: normals(T=nan), lambda: normals(T=inf),
              lambda: vertices(i=None), lambda: vertices(nr=None), lambda: vertices(o=None), lambda: vertices(i=pv + 2), lambda: vertices(nr=pn + 1),
              lambda: vertices(o=po + 2), lambda: vertices(o=pv), lambda: vertices(i=po), lambda: vertices(i=po + 12), lambda: vertices(nr=po),
              lambda: vertices(o=pn), lambda: vertices(n=257), lambda: vertices(n=0xFFFFFFFF),
              lambda: faces(off=pb + 2), lambda: faces(fc=pb + 1)):
        assert r() == -1
    dn.ctx.sync()
    assert not out.any() and not buf.any() and raw(vdev) == m["vertices"].tobytes() and raw(ndev) == nexp.tobytes()
    assert vertices() == 0 and faces() == 0
    dn.ctx.sync()
    assert raw(out[:n_v]) == denoised("noisy_cube", 2, 2, 0.4).tobytes() and not out[n_v:].any()
    assert raw(buf[:n_v + 1]) == tab["offsets"].tobytes() and not buf[n_v + 1:].any()
    still_works()
    for bad in (dict(normal_iterations=-1), dict(normal_iterations=257), dict(vertex_iterations=257), dict(threshold=1.0)):
        with pytest.raises(ValueError):                     # the Python checks come first
            dn.run(vdev, **bad)
    with pytest.raises(ValueError):
        dn.normals(vdev[:-1])
    with pytest.raises(ValueError):
        dn.vertices(vdev, ndev[:-1])
    with pytest.raises(ValueError):
        dn.normals(tri)
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        with pytest.raises(Exception):
            DN.Denoiser(dn.ctx, v, t)
    still_works()


# ---- through the volume, a tracked run and the command line -----------------------------------------------------------------------------
def mirrored(v, t, denoise, smooth=None):
    """what the surface chain makes of a mesh after the filling, from the mirrors: positions, vertex normals, the figures of both stages"""
    kw = DN.denoise_arg(denoise)
    tab = DM.face_table(t, len(v))
    out, _ = DM.denoise(v, None, tab=tab, **kw)
    figures = dict(tab["counts"], vertices=len(v), triangles=len(t), **kw)
    adj = SM.adjacency(t, len(v))
    smoothed = None
    if smooth is not None:
        skw = TS.smooth_arg(smooth)
        out = SM.smooth(out, None, skw["iterations"], skw["lam"], skw["mu"], skw["pin_boundary"], adj=adj)
        smoothed = dict(adj["counts"], vertices=len(v), triangles=len(t), **skw)
    return out, SM.normals(out, adj), figures, smoothed


def test_volume_extract_denoises(ctx):
    """a large and a small sphere in 128 x 64 x 64 voxels through Volume.extract(fill_holes=..., denoise=..., smooth=..., normals=True)
    against extract with the filling, then the mirrors: denoising after the filling and before the smoothing, the normals of the last surface"""
    m = TM.Volume(128, 64, 64, (0.0, 0.0, 0.0), 0.05, 0.2)
    big, W = TM.sphere_state(m, (3.2, 1.6, 1.6), 1.5)
    small, _ = TM.sphere_state(m, (0.4, 0.4, 0.4), 0.25)
    vol = TS.Volume(ctx, m.n, 1, colour=False)
    vol.configure(128, 64, 64, [0.0, 0.0, 0.0], 0.05, 0.2)
    vol.set_state(torch.from_numpy(np.minimum(big, small)).cuda(), torch.from_numpy(W.view(np.int32)).cuda())
    fv, fc, ft, fn = vol.extract(1, normals=True, fill_holes=16)
    filled = vol.last_fill
    hv, ht = fv.cpu().numpy(), ft.cpu().numpy().view(U32)
    ev, en, figures, smoothed = mirrored(hv, ht, dict(normal_iterations=3, vertex_iterations=4, threshold=0.5), dict(iterations=2))
    v, c, t, n = vol.extract(1, normals=True, fill_holes=16, denoise=dict(normal_iterations=3, vertex_iterations=4, threshold=0.5), smooth=2)
    assert raw(v) == ev.tobytes() and raw(n) == en.tobytes() and raw(t) == raw(ft)
    assert (c is None) == (fc is None) and (c is None or raw(c) == raw(fc))
    assert vol.last_denoise == figures and vol.last_smooth == smoothed and vol.last_fill == filled, (vol.last_denoise, figures)
    # denoising alone: with the normals of the denoised surface, and without normals
    ev, en, figures, _ = mirrored(hv, ht, 2)
    v, c, t, n = vol.extract(1, normals=True, fill_holes=16, denoise=2)
    assert raw(v) == ev.tobytes() and raw(n) == en.tobytes() and vol.last_denoise == figures and raw(v) != raw(fv)
    v, c, t = vol.extract(1, colours=False, fill_holes=16, denoise=2)
    assert c is None and raw(v) == ev.tobytes() and raw(t) == raw(ft)
    vol.close()


def test_track_dataset_mesh_denoise_option(ctx, tmp_path):
    """without the new option the PLY and the trajectory are what fuse gives today; with --mesh-denoise the file holds exactly fuse's
    denoised tensors, the trajectory and the mesh line are unchanged and one more line tells what the denoising did"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("denoised", ["--mesh-normals", "--mesh-denoise", "3", "--mesh-denoise-vertex-iterations", "4",
                                                     "--mesh-denoise-threshold", "0.5"])):
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
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_denoised.txt").read_bytes()
    v, c, t, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True)
    assert "denoise" not in info
    dv, dc, dt, dnrm, dinfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True, normals=True,
                                      denoise=dict(normal_iterations=3, vertex_iterations=4, threshold=0.5))
    ev, en, figures, _ = mirrored(v.cpu().numpy(), t.cpu().numpy().view(U32), dict(normal_iterations=3, vertex_iterations=4, threshold=0.5))
    assert dinfo["denoise"] == figures and {k: dinfo[k] for k in info} == info
    assert raw(dv) == ev.tobytes() and raw(dnrm) == en.tobytes() and raw(dt) == raw(t) and raw(dc) == raw(c) and raw(dv) != raw(v)
    assert (tmp_path / "plain.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0
    assert (tmp_path / "denoised.ply").read_bytes() == TS.mesh_ply_bytes(dv, dc, dt, dnrm)
    line = f"{info['voxels']} voxels of 0.05 m (truncation 0.2 m), {info['touched']} touched, {v.shape[0]} vertices, {t.shape[0]} triangles"
    assert line in said["plain"] and line in said["denoised"] and "mesh denoise" not in said["plain"]
    f = dinfo["denoise"]
    assert (f"mesh denoise: 3 normal iterations with threshold 0.5, 4 vertex iterations, longest row {f['longest_row']}, "
            f"{f['empty_rows']} vertices without a triangle") in said["denoised"], said["denoised"]
    other = lambda s: [l.replace("denoised.ply", "plain.ply").replace("traj_denoised", "traj_plain") for l in s.splitlines() if "mesh denoise" not in l]
    mesh_lines = lambda s: [l for l in other(s) if " mesh of " in l]
    assert mesh_lines(said["plain"]) == mesh_lines(said["denoised"]) and len(mesh_lines(said["plain"])) == 1
    assert len(said["denoised"].splitlines()) == len(said["plain"].splitlines()) + 1
