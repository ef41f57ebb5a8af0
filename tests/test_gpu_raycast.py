"""GPU tests of the TSDF ray cast and the vertex normals (include/rgbid_tsdf_raycast.h, csrc/kernels_tsdf.hip, rgbid.tsdf): the bytes of the
depth, normal and colour planes and of the vertex normals against the numpy restatement (tests/raycast_mirror.py) on the mixed volume
with cameras in front of, behind and beside it, whole and ragged pixel tiles, the threshold scene to the ulp, a handle without colour,
absent outputs, two large volumes, a plan that survives a ray cast, the refusals, a handle reused for a larger volume, a tracked run and
the options of tools/track_dataset.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import sequence, synth, tsdf as TS, tum
from rgbid.render import depth_png
from tests import raycast_mirror as RM
from tests import tsdf_mirror as TM
from tests.test_cpu_consist import COLS, K, ROWS
from tests.test_cpu_raycast import BACK, TH_CASES, mixed_state, ray_cameras, th_volume
from tests.test_cpu_tsdf import TH_K, mixed_volume
from tests.test_gpu_cloud import K_SMALL, write_tum_folder
from tests.test_gpu_tsdf import configured, mirror_of_fuse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAST = dict(z_min=0.3, z_max=5.0, step=0.05)


def loaded(ctx, mirror, max_views=32, vol=None):
    """a device volume of the mirror's shape and state (a new handle, or `vol` configured again)"""
    vol = configured(ctx, mirror, max_views, vol)
    rgb = torch.from_numpy(mirror.rgb.view(np.int32)).cuda() if mirror.colour else None
    vol.set_state(torch.from_numpy(mirror.D).cuda(), torch.from_numpy(mirror.counts().view(np.int32)).cuda(), rgb)
    return vol


def assert_planes(got, want):
    for name in ("depth", "normal"):
        g, e = got[name].cpu().numpy().view(np.uint32), want[name].view(np.uint32)
        bad = np.nonzero(g != e)
        assert bad[0].size == 0, (name, bad[0].size, [b[:5] for b in bad], g[bad][:5].view(F), e[bad][:5].view(F))
    g, e = got["colour"].cpu().numpy(), want["colour"]
    bad = np.nonzero(g != e)
    assert bad[0].size == 0, ("colour", bad[0].size, [b[:5] for b in bad], g[bad][:5], e[bad][:5])


def assert_cast(vol, mirror, R, t, K_, rows, cols, z_min, z_max, step, min_weight=1):
    """-> the mirror's planes, which the device's equal byte for byte"""
    got = vol.raycast(R, t, K_, rows, cols, step, min_weight, z_min, z_max)
    want = RM.raycast(mirror, R, t, K_, rows, cols, z_min, z_max, step, min_weight)
    assert got["depth"].shape == want["depth"].shape and got["normal"].shape == want["normal"].shape and got["colour"].shape == want["colour"].shape
    assert_planes(got, want)
    return want


def assert_normals(vol, mirror, min_weight=1):
    v, c, t, n = vol.extract(min_weight, normals=True)
    want = RM.vertex_normals(mirror, min_weight)
    assert n.shape == (len(want), 3) and v.cpu().numpy().tobytes() == TM.extract(mirror, min_weight)[0].tobytes()
    g = n.cpu().numpy()
    bad = np.nonzero((g.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (bad.size, bad[:5], g[bad[:5]], want[bad[:5]])
    return want


@pytest.mark.parametrize("V", [1, 3, 17])
def test_raycast_mixed_shapes(ctx, V):
    mirror = mixed_state()
    vol = loaded(ctx, mirror)
    R, t = ray_cameras(V)
    for rows, cols in ((ROWS, COLS), (ROWS - 1, COLS - 1)):          # whole 8 x 8 tiles, and ragged ones
        for mw in (1, 2):
            want = assert_cast(vol, mirror, R, t, K, rows, cols, min_weight=mw, **CAST)
            hits = np.isfinite(want["depth"]).reshape(V, -1).sum(1)
            assert hits[0] > 800 and want["colour"][0].any() and (want["redefined"].sum() > 0.9 * hits.sum())
            if V > 2:
                assert (want["exit_n"][1] >= 0).sum() > 800 and hits[2] == 0      # from behind: exits; from outside: nothing
    assert_normals(vol, mirror, 1)
    assert_normals(vol, mirror, 2)
    vol.close()


def test_raycast_thresholds_to_the_ulp(ctx):
    """every view of every case of the threshold scene alone (tests/test_cpu_raycast.py asserts what each of them is about), then a
    case's views in one call"""
    vol = None
    for name, c in TH_CASES.items():
        mirror = th_volume(c["kind"])
        vol = loaded(ctx, mirror, vol=vol)
        R, t = np.stack([v[0] for v in c["views"]]), np.array([v[1] for v in c["views"]], np.float64)
        for sel in [[v] for v in range(len(R))] + [list(range(len(R)))]:
            assert_cast(vol, mirror, R[sel], t[sel], TH_K, ROWS, COLS, c["z_min"], c["z_max"], c["step"], c["min_weight"])
        assert_normals(vol, mirror, c["min_weight"])
    vol.close()


def test_raycast_without_colour_and_absent_outputs(ctx):
    R, t = ray_cameras(3)
    plain = mixed_volume(colour=False)
    plain.set_state(mixed_state().D, mixed_state().counts() & np.uint32(0xFFFF))
    vol = loaded(ctx, plain)
    want = assert_cast(vol, plain, R, t, K, ROWS, COLS, **CAST)
    assert np.isfinite(want["depth"]).sum() > 800 and not want["colour"].any()
    vol.close()
    # each output absent in turn, and a canary behind every buffer
    mirror = mixed_state()
    vol = loaded(ctx, mirror)
    want = RM.raycast(mirror, R, t, K, ROWS - 1, COLS - 1, min_weight=1, **CAST)
    P = 3 * (ROWS - 1) * (COLS - 1)
    for absent in (None, "depth", "normal", "colour"):
        depth = torch.full((P + 16,), 7.0, dtype=torch.float32, device="cuda")
        normal = torch.full((3 * P + 16,), 7.0, dtype=torch.float32, device="cuda")
        colour = torch.full((3 * P + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        planes = dict(depth=depth[:P].view(3, ROWS - 1, COLS - 1), normal=normal[:3 * P].view(3, 3, ROWS - 1, COLS - 1),
                      colour=colour[:3 * P].view(3, ROWS - 1, COLS - 1, 3))
        given = {k: (None if k == absent else x) for k, x in planes.items()}
        ctx.wait_torch_stream()
        vol.raycast_into(R, t, K, ROWS - 1, COLS - 1, 0.05, 1, 0.3, 5.0, **given)
        ctx.sync()
        assert (depth[P:] == 7.0).all() and (normal[3 * P:] == 7.0).all() and (colour[3 * P:] == 0xA5).all()
        for k, x in planes.items():
            if k == absent:
                assert (x == (0xA5 if k == "colour" else 7.0)).all()
            else:
                assert x.cpu().numpy().tobytes() == want[k].tobytes(), (absent, k)
    ctx.wait_torch_stream()
    vol.raycast_into(R, t, K, ROWS, COLS, 0.05, 1, 0.3, 5.0)     # nothing asked for: a valid call
    ctx.sync()
    vol.close()


@pytest.mark.parametrize("nx", [128, 129])
def test_raycast_large_sphere(ctx, nx):
    """a sphere of 1.5 m in nx x 64 x 64 voxels seen in 3 views of 120 x 160 pixels from in front, from behind and from the side: every
    third of each image has hits; the vertex normals of its mesh as well"""
    sphere = TM.Volume(nx, 64, 64, (0.0, 0.0, 0.0), 0.05, 0.2)
    sphere.set_state(*TM.sphere_state(sphere, (nx * 0.025, 1.6, 1.6), 1.5))
    vol = loaded(ctx, sphere)
    side = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])      # R_WC of a camera that looks along the world's -x (its x axis is the world's z)
    R = np.stack([np.eye(3), BACK, side])
    t = np.array([[nx * 0.025, 1.6, -2.4], [nx * 0.025, 1.6, 5.6], [nx * 0.025 + 4.0, 1.6, 1.6]])
    Kl = (100.0, 100.0, 79.5, 59.5)
    want = assert_cast(vol, sphere, R, t, Kl, 120, 160, 0.3, 8.0, 0.05)
    hit = np.isfinite(want["depth"])
    for v in range(3):
        for a in range(3):
            assert hit[v, 40 * a:40 * (a + 1)].sum() > 500, (v, a, int(hit[v, 40 * a:40 * (a + 1)].sum()))
    n = assert_normals(vol, sphere, 1)
    assert len(n) > 25_000
    vol.close()


def test_plan_survives_a_raycast_and_a_larger_volume_follows_a_smaller(ctx):
    small = TM.Volume(9, 7, 5, (-0.2, -0.15, 1.6), 0.05, 0.15)
    src = mixed_state()
    small.set_state(src.D[5:10, 6:13, 7:16], src.counts()[5:10, 6:13, 7:16], src.rgb[:, 5:10, 6:13, 7:16])
    vol = TS.Volume(ctx, src.n, 4)
    loaded(ctx, small, vol=vol)
    R, t = ray_cameras(3)
    assert_cast(vol, small, R, t, K, ROWS, COLS, **CAST)
    assert_normals(vol, small, 1)
    mirror = mixed_state()                                   # the larger volume on the same handle
    loaded(ctx, mirror, vol=vol)
    ev, ec, et = TM.extract(mirror, 1)
    nv, nt = C.c_ulonglong(), C.c_ulonglong()
    ctx.wait_torch_stream()
    assert vol.L.rgbid_tsdf_extract_plan(vol._h, 1, C.byref(nv), C.byref(nt)) == 0 and (nv.value, nt.value) == (len(ev), len(et))
    assert_cast(vol, mirror, R, t, K, ROWS, COLS, **CAST)    # reads the state only
    verts = torch.empty((len(ev), 3), dtype=torch.float32, device="cuda")
    cols = torch.empty((len(ev), 3), dtype=torch.uint8, device="cuda")
    tris = torch.empty((len(et), 3), dtype=torch.int32, device="cuda")
    nrm = torch.full((len(ev) + 1, 3), 7.0, dtype=torch.float32, device="cuda")
    ctx.wait_torch_stream()
    vol.emit(verts, cols, tris)
    with pytest.raises(Exception, match="rgbid error -1"):
        vol.emit_normals(nrm[:len(ev) - 1])                  # a capacity one below the plan's
    assert vol.L.rgbid_tsdf_extract_normals(vol._h, nrm.data_ptr() + 2, len(ev)) == -1 and vol.L.rgbid_tsdf_extract_normals(vol._h, None, len(ev)) == -1
    ctx.sync()
    assert (nrm == 7.0).all()
    vol.emit_normals(nrm[:len(ev)])                          # exactly the plan's
    ctx.sync()
    assert verts.cpu().numpy().tobytes() == ev.tobytes() and cols.cpu().numpy().tobytes() == ec.tobytes()
    assert tris.cpu().numpy().view(np.uint32).tobytes() == et.tobytes()
    assert nrm[:len(ev)].cpu().numpy().tobytes() == RM.vertex_normals(mirror, 1).tobytes() and (nrm[len(ev)] == 7.0).all()
    vol.reset()                                              # a plan does not outlive the state it counted
    with pytest.raises(Exception, match="rgbid error -1"):
        vol.emit_normals(nrm)
    vol.close()


def test_raycast_refusals_and_reuse(ctx):
    mirror = mixed_state()
    vol = loaded(ctx, mirror, max_views=3)
    L = vol.L
    R, t = ray_cameras(3)
    P = 3 * ROWS * COLS
    depth = torch.full((P + 1,), 7.0, dtype=torch.float32, device="cuda")
    normal = torch.full((3 * P + 1,), 7.0, dtype=torch.float32, device="cuda")
    colour = torch.full((3 * P,), 0xA5, dtype=torch.uint8, device="cuda")

    def pose_table(R_=R, t_=t, V=3):
        return (TS.Pose * V)(*[TS.Pose((C.c_double * 9)(*np.asarray(R_[v], np.float64).reshape(9)), (C.c_double * 3)(*t_[v])) for v in range(V)])

    def cast(V=3, poses=None, K_=K, rows=ROWS, cols=COLS, z_min=0.3, z_max=5.0, step=0.05, mw=1, d=0, n=0):
        ctx.wait_torch_stream()
        return L.rgbid_tsdf_raycast(vol._h, V, pose_table() if poses is None else poses, (C.c_float * 4)(*K_), rows, cols, z_min, z_max, step, mw,
                                    depth.data_ptr() + d, normal.data_ptr() + n, colour.data_ptr())

    nan, inf = float("nan"), float("inf")
    Rn = R.copy(); Rn[1, 0, 0] = nan
    ti = t.copy(); ti[2, 1] = inf
    tb = t.copy(); tb[0, 0] = 1e39                          # finite as double, infinite as float32
    refusals = [lambda: cast(V=0), lambda: cast(V=4), lambda: cast(V=-1), lambda: cast(rows=0), lambda: cast(cols=0), lambda: cast(rows=-3),
                lambda: cast(cols=(1 << 20) + 1), lambda: cast(rows=1 << 15, cols=1 << 15), lambda: cast(rows=1 << 20, cols=1 << 10),
                lambda: cast(z_min=0.0), lambda: cast(z_min=-1.0), lambda: cast(z_min=nan), lambda: cast(z_max=nan), lambda: cast(z_max=inf),
                lambda: cast(z_min=2.0, z_max=1.0), lambda: cast(step=0.0), lambda: cast(step=-0.05), lambda: cast(step=nan), lambda: cast(step=inf),
                lambda: cast(step=4.7 / 65537), lambda: cast(mw=0), lambda: cast(mw=65536),
                lambda: cast(poses=pose_table(R_=Rn)), lambda: cast(poses=pose_table(t_=ti)), lambda: cast(poses=pose_table(t_=tb)),
                lambda: cast(K_=(nan, 58.0, 31.5, 23.5)), lambda: cast(K_=(60.0, 58.0, inf, 23.5)), lambda: cast(K_=(0.0, 58.0, 31.5, 23.5)),
                lambda: cast(K_=(60.0, 0.0, 31.5, 23.5)), lambda: cast(d=2), lambda: cast(n=2)]

    def still_works():
        assert_cast(vol, mirror, R, t, K, ROWS - 1, COLS - 1, **CAST)

    still_works()
    before = [x.clone() for x in vol.state()]
    for i, r in enumerate(refusals):
        assert r() == -1, i
    ctx.sync()
    assert (depth == 7.0).all() and (normal == 7.0).all() and (colour == 0xA5).all()      # the outputs are untouched
    for a, b in zip(before, vol.state()):
        assert torch.equal(a, b)
    still_works()
    for i in (0, 8, 15, 19, 22, 29):                        # the handle is usable after each kind of refusal, not only after all
        assert refusals[i]() == -1, i
        still_works()
    assert cast(step=4.7 / 65535) == 0                      # just inside the bound on the steps: 65 535 samples, most of them skipped
    ctx.sync()
    for bad in (dict(z_min=0), dict(R=Rn), dict(K=(0, 1, 1, 1)), dict(rows=0), dict(step=0.0), dict(min_weight=0), dict(R=np.stack([np.eye(3)] * 4), t=np.zeros((4, 3)))):
        a = dict(R=R, t=t, K=K, rows=ROWS, cols=COLS)
        a.update(bad)
        with pytest.raises(ValueError):                    # the Python checks come first
            vol.raycast(**a)
    vol.timing(True)
    still_works()
    ms = vol.raycast_timing(False)
    print("tsdf ray cast ms:", ms)
    assert np.isfinite(ms) and ms > 0
    vol.close()


# ---- a tracked run and the command line -----------------------------------------------------------------------------------------------
def test_raycast_on_a_tracked_run(ctx):
    """the tracked run of tests/test_gpu_tsdf.py (2 chunks, 160 x 120, voxel 0.04 m): the volume `fuse` keeps, ray-cast at three of its
    keyframes, equals the mirror's bytes, and so do the vertex normals.  The agreement with the keyframes is printed, not asserted."""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                         keyframe_colour=True)
    kfs = pc.keyframes
    v, c, t, nrm, info, vol = TS.fuse(ctx, kfs, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, normals=True, keep_volume=True)
    try:
        mirror = mirror_of_fuse(pc, info, 0.04, 0.16, K_SMALL)
        assert v.cpu().numpy().tobytes() == TM.extract(mirror, 1)[0].tobytes()
        assert nrm.cpu().numpy().tobytes() == RM.vertex_normals(mirror, 1).tobytes() and len(nrm) > 1000
        pick = [0, len(kfs) // 2, len(kfs) - 1]
        R, tt = np.stack([kfs[i]["R"] for i in pick]), np.stack([kfs[i]["t"] for i in pick])
        want = assert_cast(vol, mirror, R, tt, K_SMALL, rows, cols, 0.05, 6.0, 0.04)
        assert np.isfinite(want["depth"]).sum() > 3 * 5000 and want["colour"].any()
        figures = TS.surface_agreement(vol, kfs, K_SMALL, rows, cols, z_max=6.0)
        run = TS.agreement_summary(figures)
        print(f"tracked run: {len(kfs)} keyframes ray-cast: {run['pixels']} pixels, median of medians {run['median']:.6f} m, largest 90 % {run['p90']:.6f} m")
        assert len(figures) == len(kfs)
    finally:
        vol.close()


def test_track_dataset_mesh_render_options(ctx, tmp_path):
    """--mesh without the new options writes what it wrote; with --mesh-normals the PLY holds fuse(normals=True)'s tensors; with
    --mesh-render the PNGs hold exactly raycast's planes"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    views = tmp_path / "views"
    said = {}
    for name, extra in (("plain", []), ("new", ["--mesh-normals", "--mesh-render", str(views), "--mesh-render-check", "--mesh-render-step", "0.04"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply"), "--mesh-voxel", "0.05"] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = r.stdout
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True, keyframe_colour=True)
    kfs = pc.keyframes
    v, c, t, nrm, vol = TS.fuse(ctx, kfs, K_SMALL, rows, cols, voxel=0.05, points=pc.points, normals=True, keep_volume=True)
    try:
        assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_new.txt").read_bytes()
        assert (tmp_path / "plain.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0
        assert (tmp_path / "new.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t, nrm)
        assert "ray-cast" not in said["plain"] and "mesh render check" not in said["plain"]
        assert "mesh render check: " in said["new"] and f"{len(kfs)} ray-cast views of the volume" in said["new"]
        names = [f"view_{i:04d}" for i in range(len(kfs))]
        assert sorted(os.listdir(views)) == sorted([x + e for x in names for e in (".png", "_depth.png", "_shaded.png")])
        want = vol.raycast(np.stack([k["R"] for k in kfs]), np.stack([k["t"] for k in kfs]), K_SMALL, rows, cols, 0.04)
        assert torch.isfinite(want["depth"]).sum() > 5000
        for i, x in enumerate(names):
            assert np.array_equal(tum.read_png(str(views / (x + ".png"))), want["colour"][i].cpu().numpy()), i
            assert np.array_equal(tum.read_png(str(views / (x + "_depth.png"))), depth_png(want["depth"][i])), i
            assert np.array_equal(tum.read_png(str(views / (x + "_shaded.png"))), TS.shade(want["normal"][i])), i
    finally:
        vol.close()
