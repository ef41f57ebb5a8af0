"""GPU tests of the TSDF volume (include/rgbid_tsdf.h, csrc/kernels_tsdf.hip, rgbid.tsdf): the state bytes, the vertex and triangle counts
and the vertex, colour and triangle bytes against the numpy restatement (tests/tsdf_mirror.py) on a volume of unequal dimensions with
planes that hold every kind of hole, either side of the view chunk, the thresholds to the ulp, views without colour, integration in
pieces, a handle reused for a smaller volume, one grid of the strided kernels and one row more, the refusals, the empty volume, a tracked
run and the options of tools/track_dataset.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import cloud as CL
from rgbid import sequence, synth, tsdf as TS, tum
from tests import tsdf_mirror as TM
from tests.test_cpu_consist import COLS, K, ROWS
from tests.test_cpu_tsdf import (GATE, HALF, TH_GATE, TH_GRID, TH_K, assert_every_third_has_work, large_scene, large_volume, mixed_scene, mixed_volume,
                                 sphere_volume, threshold_scene)
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def configured(ctx, mirror, max_views=32, vol=None):
    """a device volume of the mirror's shape (a new handle, or `vol` configured again)"""
    vol = TS.Volume(ctx, mirror.n, max_views, colour=mirror.colour) if vol is None else vol
    vol.configure(mirror.nx, mirror.ny, mirror.nz, [float(v) for v in mirror.origin], float(mirror.voxel), float(mirror.trunc))
    return vol


def upload(sc, colours=None):
    cols = sc["colours"] if colours is None else colours
    return torch.from_numpy(np.ascontiguousarray(sc["planes"], F)).cuda(), [None if c is None else torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


def both(vol, mirror, sc, dplanes, dcols, cols, a, b, K_=K, gate=GATE):
    """views a .. b - 1 into the device volume and into the mirror"""
    vol.integrate(dplanes[a:b], dcols[a:b], sc["R"][a:b], sc["t"][a:b], K_, dplanes.shape[1], dplanes.shape[2], **gate)
    TM.integrate(mirror, sc["planes"][a:b], cols[a:b], sc["R"][a:b], sc["t"][a:b], K_, **gate)


def assert_state(vol, mirror):
    D, counts, rgb = (x.cpu().numpy() for x in vol.state())
    eD, ec, ergb = mirror.D, mirror.counts(), mirror.rgb
    bad = np.nonzero((D.view(np.uint32) != eD.view(np.uint32)) | (counts.view(np.uint32) != ec))
    assert bad[0].size == 0, (bad[0].size, [b[:5] for b in bad], D[bad][:5], eD[bad][:5], counts[bad][:5], ec[bad][:5])
    assert rgb.view(np.uint32).tobytes() == ergb.tobytes()
    assert D.shape == mirror.shape and rgb.shape == (3,) + mirror.shape


def assert_mesh(vol, mirror, min_weight=1):
    """-> the mirror's (vertices, colours, triangles), which the device's equal byte for byte"""
    v, c, t = vol.extract(min_weight)
    ev, ec, et = TM.extract(mirror, min_weight)
    assert (v.shape[0], t.shape[0]) == (len(ev), len(et)), (v.shape, t.shape, len(ev), len(et))
    gv, gt = v.cpu().numpy(), t.cpu().numpy().view(np.uint32)
    bad = np.nonzero((gv.view(np.uint32) != ev.view(np.uint32)).any(1))[0]
    assert bad.size == 0, (bad.size, bad[:5], gv[bad[:5]], ev[bad[:5]])
    assert c.cpu().numpy().tobytes() == ec.tobytes()
    bad = np.nonzero((gt != et).any(1))[0]
    assert bad.size == 0, (bad.size, bad[:5], gt[bad[:5]], et[bad[:5]])
    return ev, ec, et


@pytest.mark.parametrize("V", [3, 19])
def test_tsdf_mixed_shapes(ctx, V):
    sc = mixed_scene(V)
    for kind in (np.nan, 0.0, -0.5, np.inf, 1e-39):
        assert (sc["planes"] == F(kind)).any() or (np.isnan(kind) and np.isnan(sc["planes"]).any())
    dplanes, dcols = upload(sc)
    mirror = mixed_volume()
    vol = configured(ctx, mirror)
    both(vol, mirror, sc, dplanes, dcols, sc["colours"], 0, V)
    assert_state(vol, mirror)
    assert mirror.W.max() >= min(V, 10) and (mirror.W == 0).any() and (mirror.Cn < mirror.W).any()
    for mw in (1, 2):
        ev, ec, et = assert_mesh(vol, mirror, mw)
        assert len(ev) > 300 and len(et) > 500 and ec.any()
    v, c, t = vol.extract(1, colours=False)                # the colour buffer may be absent
    assert c is None and v.cpu().numpy().tobytes() == TM.extract(mirror, 1)[0].tobytes()
    vol.close()


def test_tsdf_either_side_of_the_view_chunk(ctx):
    """exactly VIEW_CHUNK views are one launch, one more a second launch after it; a view moved across the boundary changes the result
    exactly as it changes the mirror's, because the running mean depends on the order"""
    V = TS.VIEW_CHUNK + 1
    sc = mixed_scene(19)
    dplanes, dcols = upload(sc)
    seen = []
    for order in (list(range(V - 1)), list(range(V)), [V - 1] + list(range(V - 1)), list(range(1, V)) + [0]):
        sub = dict(R=sc["R"][order], t=sc["t"][order], planes=sc["planes"][order])
        cols = [sc["colours"][i] for i in order]
        mirror = mixed_volume()
        vol = configured(ctx, mirror)
        both(vol, mirror, sub, dplanes[order], [dcols[i] for i in order], cols, 0, len(order))
        assert_state(vol, mirror)
        assert_mesh(vol, mirror, 2)
        seen.append(mirror.D.tobytes())
        vol.close()
    assert len(set(seen)) == 4


def test_tsdf_thresholds_to_the_ulp(ctx):
    """s on -trunc and +trunc and one ulp either side, Z on each gate and one ulp outside, pu and pv on each image border: every view alone
    (tests/test_cpu_tsdf.py asserts what each of them does to the voxels it is about), then all in one call"""
    sc = threshold_scene()
    dplanes, dcols = upload(sc)
    V = len(sc["R"])
    vol = None
    for a, b in [(v, v + 1) for v in range(V)] + [(0, V)]:
        mirror = TM.Volume(**TH_GRID)
        vol = configured(ctx, mirror, vol=vol)
        both(vol, mirror, sc, dplanes, dcols, sc["colours"], a, b, TH_K, TH_GATE)
        assert_state(vol, mirror)
    assert_mesh(vol, mirror, 1)
    vol.close()


def test_tsdf_views_without_colour(ctx):
    sc = mixed_scene(19)
    cols = list(sc["colours"])
    for i in (0, 5, 16, 18):
        cols[i] = None
    dplanes, dcols = upload(sc, cols)
    mirror = mixed_volume()
    vol = configured(ctx, mirror)
    both(vol, mirror, sc, dplanes, dcols, cols, 0, 19)
    assert_state(vol, mirror)
    assert_mesh(vol, mirror, 1)
    assert (mirror.Cn > 0).any() and mirror.Cn.max() <= 15
    vol.close()
    # a handle without colour: eight bytes of state per voxel, every view taken as colourless, a black mesh
    mirror = mixed_volume(colour=False)
    vol = configured(ctx, mirror)
    both(vol, mirror, sc, dplanes, dcols, cols, 0, 19)
    assert_state(vol, mirror)
    ev, ec, et = assert_mesh(vol, mirror, 1)
    assert not mirror.Cn.any() and not ec.any() and len(et) > 500
    with pytest.raises(ValueError):
        vol.set_state(*vol.state())
    vol.close()


def test_tsdf_integrating_in_pieces(ctx):
    sc = mixed_scene(19)
    dplanes, dcols = upload(sc)
    whole = TM.integrate(mixed_volume(), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)
    mirror = mixed_volume()
    vol = configured(ctx, mirror)
    for a, b in ((0, 1), (1, 7), (7, 19)):
        both(vol, mirror, sc, dplanes, dcols, sc["colours"], a, b)
    assert mirror.state_bytes() == whole.state_bytes()
    assert_state(vol, mirror)
    assert_mesh(vol, mirror, 3)
    vol.close()


def test_tsdf_state_round_trip_and_reuse(ctx):
    """set_state(get_state) changes nothing; reset and configure to a smaller volume after a larger one leave nothing of the larger behind"""
    sc = mixed_scene(3)
    dplanes, dcols = upload(sc)
    mirror = mixed_volume()
    vol = configured(ctx, mirror)
    both(vol, mirror, sc, dplanes, dcols, sc["colours"], 0, 3)
    D, counts, rgb = vol.state()
    assert_mesh(vol, mirror, 1)
    vol.reset()
    empty = mixed_volume()
    assert_state(vol, empty)
    assert_mesh(vol, empty, 1)
    vol.set_state(D, counts, rgb)
    assert_state(vol, mirror)
    assert_mesh(vol, mirror, 1)
    vol.set_state(D, counts)                               # without sums: zeros
    mirror.set_state(mirror.D, mirror.counts())
    assert_state(vol, mirror)
    ev, ec, et = assert_mesh(vol, mirror, 1)
    assert mirror.Cn.any() and not ec.any()
    small = TM.Volume(9, 7, 5, (-0.2, -0.15, 1.6), 0.05, 0.15)      # a smaller volume on the same handle
    configured(ctx, small, vol=vol)
    assert_state(vol, small)
    both(vol, small, sc, dplanes, dcols, sc["colours"], 0, 3)
    assert_state(vol, small)
    ev, _, et = assert_mesh(vol, small, 1)
    assert len(ev) > 20 and len(et) > 20
    sphere = sphere_volume()                                # the larger shape again, with a state of its own
    configured(ctx, sphere, vol=vol)
    vol.set_state(torch.from_numpy(sphere.D).cuda(), torch.from_numpy(sphere.counts().view(np.int32)).cuda())
    assert_state(vol, sphere)
    ev, _, et = assert_mesh(vol, sphere, 1)
    assert (len(ev), len(et)) == (2002, 4000)
    vol.close()


@pytest.mark.parametrize("nx", [128, 129])
def test_tsdf_either_side_of_one_grid(ctx, nx):
    """128 x 64 x 64 voxels: every thread makes one trip; 129: a second trip of the first 4 096 threads, lanes of the last wave differ.  The
    7 n edge flags are 1 792 tiles and more: k_vox_scan1 makes seven trips.  The sphere state is extracted at both sizes as well."""
    sc = large_scene()
    dplanes, dcols = upload(sc)
    mirror = large_volume(nx)
    assert (mirror.n == HALF) == (nx == 128)
    vol = configured(ctx, mirror)
    both(vol, mirror, sc, dplanes, dcols, sc["colours"], 0, 3)
    assert_state(vol, mirror)
    ev, ec, et = assert_mesh(vol, mirror, 1)
    print(f"{nx} x 64 x 64, 3 views: {int((mirror.W > 0).sum())} voxels touched, {len(ev)} vertices, {len(et)} triangles")
    assert_every_third_has_work(mirror, ev, et)
    sphere = TM.Volume(nx, 64, 64, (0.0, 0.0, 0.0), 0.05, 0.2)
    sphere.set_state(*TM.sphere_state(sphere, (nx * 0.025, 1.6, 1.6), 1.5))
    configured(ctx, sphere, vol=vol)
    vol.set_state(torch.from_numpy(sphere.D).cuda(), torch.from_numpy(sphere.counts().view(np.int32)).cuda())
    ev, _, et = assert_mesh(vol, sphere, 1)
    edges, two, repeated = TM.mesh_topology(et)
    assert two == edges and repeated == 0 and len(ev) - edges + len(et) == 2 and len(et) > 50_000
    z = ev[:, 2]
    for lo, hi in ((0.0, 1.1), (1.1, 2.1), (2.1, 3.2)):
        assert ((z >= lo) & (z < hi)).sum() > 5000
    vol.close()


def test_tsdf_refusals_and_reuse(ctx):
    sc = mixed_scene(3)
    dplanes, dcols = upload(sc)
    mirror = mixed_volume()
    vol = configured(ctx, mirror, max_views=3)
    L = vol.L
    R, t = sc["R"], sc["t"]

    def views(R_=R, t_=t, planes=None, cols=None):
        planes = [p.data_ptr() for p in dplanes] if planes is None else planes
        cols = [c.data_ptr() for c in dcols] if cols is None else cols
        return (TS.View * len(planes))(*[TS.View(TS.Pose((C.c_double * 9)(*np.asarray(R_[v], np.float64).reshape(9)), (C.c_double * 3)(*t_[v])),
                                                 planes[v], cols[v]) for v in range(len(planes))])

    def integrate(V=3, vw=None, K_=K, rows=ROWS, cols=COLS, z_min=0.3, z_max=5.0):
        ctx.wait_torch_stream()
        return L.rgbid_tsdf_integrate(vol._h, V, views() if vw is None else vw, (C.c_float * 4)(*K_), rows, cols, z_min, z_max)

    def configure(nx=24, ny=20, nz=16, origin=(0.0, 0.0, 0.0), voxel=0.05, trunc=0.15):
        return L.rgbid_tsdf_configure(vol._h, nx, ny, nz, (C.c_float * 3)(*origin), voxel, trunc)

    def still_works():
        m = mixed_volume()
        configured(ctx, m, vol=vol)
        both(vol, m, sc, dplanes, dcols, sc["colours"], 0, 3)
        assert_state(vol, m)
        assert_mesh(vol, m, 1)

    nan, inf = float("nan"), float("inf")
    Rn = R.copy(); Rn[1, 0, 0] = nan
    ti = t.copy(); ti[2, 1] = inf
    tb = t.copy(); tb[0, 0] = 1e39                          # finite as double, infinite as float32
    p = [x.data_ptr() for x in dplanes]
    nv, nt = C.c_ulonglong(), C.c_ulonglong()
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    refusals = [lambda: configure(nx=1), lambda: configure(ny=1), lambda: configure(nz=1), lambda: configure(nx=25), lambda: configure(nz=-16),
                lambda: configure(voxel=0.0), lambda: configure(voxel=-0.05), lambda: configure(voxel=nan), lambda: configure(voxel=inf),
                lambda: configure(trunc=0.0), lambda: configure(trunc=-0.1), lambda: configure(trunc=nan), lambda: configure(trunc=inf),
                lambda: configure(origin=(nan, 0, 0)), lambda: configure(origin=(0, inf, 0)), lambda: configure(origin=(0, 0, -inf)),
                lambda: integrate(V=0), lambda: integrate(V=4), lambda: integrate(V=-1),
                lambda: integrate(rows=0), lambda: integrate(cols=0), lambda: integrate(rows=-3), lambda: integrate(cols=(1 << 20) + 1),
                lambda: integrate(z_min=0.0), lambda: integrate(z_min=-1.0), lambda: integrate(z_min=nan), lambda: integrate(z_max=nan),
                lambda: integrate(z_max=inf), lambda: integrate(z_min=2.0, z_max=1.0),
                lambda: integrate(vw=views(R_=Rn)), lambda: integrate(vw=views(t_=ti)), lambda: integrate(vw=views(t_=tb)),
                lambda: integrate(K_=(nan, 58.0, 31.5, 23.5)), lambda: integrate(K_=(60.0, 58.0, inf, 23.5)), lambda: integrate(K_=(0.0, 58.0, 31.5, 23.5)),
                lambda: integrate(K_=(60.0, 0.0, 31.5, 23.5)),
                lambda: integrate(vw=views(planes=[p[0], 0, p[2]])), lambda: integrate(vw=views(planes=[p[0] + 2, p[1], p[2]])),
                lambda: L.rgbid_tsdf_extract_plan(vol._h, 0, C.byref(nv), C.byref(nt)), lambda: L.rgbid_tsdf_extract_plan(vol._h, 65536, C.byref(nv), C.byref(nt)),
                lambda: L.rgbid_tsdf_get_state(vol._h, buf.data_ptr() + 2, None, None), lambda: L.rgbid_tsdf_get_state(vol._h, None, buf.data_ptr() + 1, None),
                lambda: L.rgbid_tsdf_set_state(vol._h, None, None, buf.data_ptr() + 2)]
    still_works()
    before = [x.clone() for x in vol.state()]
    for i, r in enumerate(refusals):
        assert r() == -1, i
    for a, b in zip(before, vol.state()):                  # a refusal changes nothing, not even the shape
        assert torch.equal(a, b)
    still_works()
    for i in (0, 16, 24, 36):                              # the handle is usable after each kind of refusal, not only after all
        assert refusals[i]() == -1, i
        still_works()
    for bad in (dict(z_min=0), dict(R=Rn), dict(K=(0, 1, 1, 1)), dict(rows=0), dict(z_min=3.0, z_max=2.0)):
        a = dict(planes=dplanes, colours=dcols, R=R, t=t, K=K, rows=ROWS, cols=COLS)
        a.update(bad)
        with pytest.raises(ValueError):                    # the Python checks come first
            vol.integrate(**a)
    with pytest.raises(ValueError):
        vol.integrate(dplanes[:, :, :COLS - 1].contiguous(), dcols, R, t, K, ROWS, COLS)
    with pytest.raises(ValueError):
        vol.integrate(dplanes, [c[:, :, :2].contiguous() for c in dcols], R, t, K, ROWS, COLS)
    # the emit: misaligned outputs, capacities below the plan's, and exactly the plan's with a canary behind
    still_works()
    ev, ec, et = TM.extract(TM.integrate(mixed_volume(), sc["planes"], sc["colours"], R, t, K, **GATE), 1)
    assert L.rgbid_tsdf_extract_plan(vol._h, 1, C.byref(nv), C.byref(nt)) == 0 and (nv.value, nt.value) == (len(ev), len(et))
    verts = torch.full((len(ev) + 1, 3), 7.0, dtype=torch.float32, device="cuda")
    cols = torch.full((len(ev) + 1, 3), 0xA5, dtype=torch.uint8, device="cuda")
    tris = torch.full((len(et) + 1, 3), -7, dtype=torch.int32, device="cuda")
    ctx.wait_torch_stream()
    with pytest.raises(Exception, match="rgbid error -1"):
        vol.emit(verts[:len(ev) - 1], cols[:len(ev) - 1], tris)
    with pytest.raises(Exception, match="rgbid error -1"):
        vol.emit(verts, cols, tris[:len(et) - 1])
    emit = lambda v, t_: L.rgbid_tsdf_extract_emit(vol._h, v, cols.data_ptr(), t_, len(ev), len(et))
    assert emit(verts.data_ptr() + 2, tris.data_ptr()) == -1 and emit(verts.data_ptr(), tris.data_ptr() + 2) == -1
    assert emit(None, tris.data_ptr()) == -1 and emit(verts.data_ptr(), None) == -1
    ctx.sync()
    assert (verts == 7.0).all() and (cols == 0xA5).all() and (tris == -7).all()
    vol.emit(verts[:len(ev)], cols[:len(ev)], tris[:len(et)])
    ctx.sync()
    assert (verts[len(ev)] == 7.0).all() and (cols[len(ev)] == 0xA5).all() and (tris[len(et)] == -7).all()
    assert verts[:len(ev)].cpu().numpy().tobytes() == ev.tobytes() and cols[:len(ev)].cpu().numpy().tobytes() == ec.tobytes()
    assert tris[:len(et)].cpu().numpy().view(np.uint32).tobytes() == et.tobytes()
    vol.reset()                                            # a plan does not outlive the state it counted
    with pytest.raises(Exception, match="rgbid error -1"):
        vol.emit(verts, cols, tris)
    vol.timing(True)
    still_works()
    ms = vol.timing(False)
    print("tsdf stage ms:", ms)
    assert tuple(ms) == TS.STAGES and all(np.isfinite(v) and v >= 0 for v in ms.values()) and sum(ms.values()) > 0
    vol.close()
    for mv, mw in ((7, 2), ((1 << 29) + 1, 2), (1000, 0), (1000, 65536)):
        with pytest.raises(Exception):
            TS.Volume(ctx, mv, mw)


def test_tsdf_empty_volume(ctx):
    mirror = mixed_volume()
    vol = configured(ctx, mirror)
    ev, ec, et = assert_mesh(vol, mirror, 1)               # nothing integrated: no valid voxel
    assert len(ev) == 0 and len(et) == 0
    v, c, t = vol.extract(1)
    assert v.shape == (0, 3) and c.shape == (0, 3) and t.shape == (0, 3)
    sc = mixed_scene(3)
    dplanes, dcols = upload(sc)
    far = dict(sc, t=sc["t"] + np.array([0, 0, 50.0]))      # every voxel behind the cameras
    both(vol, mirror, far, dplanes, dcols, sc["colours"], 0, 3)
    assert_state(vol, mirror)
    assert not mirror.W.any()
    assert len(assert_mesh(vol, mirror, 1)[0]) == 0
    vol.close()


# ---- a tracked run and the command line -----------------------------------------------------------------------------------------------
def mirror_of_fuse(pc, info, voxel, trunc, K_, colour=True):
    mirror = TM.Volume(info["nx"], info["ny"], info["nz"], info["origin"], voxel, trunc, colour=colour)
    kfs = pc.keyframes
    TM.integrate(mirror, [k["depthinv"].cpu().numpy() for k in kfs], [k["colour"].cpu().numpy() for k in kfs], np.stack([k["R"] for k in kfs]),
                 np.stack([k["t"] for k in kfs]), K_, 0.05, 20.0)
    return mirror


def test_tsdf_on_a_tracked_run(ctx):
    """the 2-chunk noise-free synthetic run of tests/test_gpu_render.py at 160 x 120 with the keyframes' depth and colours kept: `fuse` at
    a 0.04 m voxel equals the mirror's bytes.  The mesh's figures are printed, not asserted (DESIGN.md section 19 holds the measured ones)."""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                         keyframe_colour=True)
    kfs = pc.keyframes
    assert len(kfs) >= 3 and all(k["colour"].shape == (rows, cols, 3) and k["colour"].dtype == torch.uint8 for k in kfs)
    # the kept colours are the ones the cloud's records carry
    p = pc.numpy()
    first = p[int(pc.offsets[0]):int(pc.offsets[1])]
    col0 = kfs[0]["colour"].cpu().numpy().reshape(-1, 3)[first["pixel"]]
    assert len(first) > 1000 and np.array_equal(col0, np.stack([first["r"], first["g"], first["b"]], 1))
    v, c, t, info = TS.fuse(ctx, kfs, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True)
    mirror = mirror_of_fuse(pc, info, 0.04, 0.16, K_SMALL)
    ev, ec, et = TM.extract(mirror, 1)
    assert info["voxels"] == mirror.n and info["touched"] == int((mirror.W > 0).sum()) > 1000
    assert v.cpu().numpy().tobytes() == ev.tobytes() and c.cpu().numpy().tobytes() == ec.tobytes()
    assert t.cpu().numpy().view(np.uint32).tobytes() == et.tobytes() and len(et) > 1000
    edges, two, _ = TM.mesh_topology(et)
    print(f"tracked run: {len(kfs)} keyframes into {info['nx']} x {info['ny']} x {info['nz']} voxels of 0.04 m, {info['touched']} touched: "
          f"{len(ev)} vertices, {len(et)} triangles, {two / max(edges, 1):.4f} of {edges} edges in two triangles")


def test_track_dataset_mesh_options(ctx, tmp_path):
    """without --mesh the trajectory and the PLY are what they were: the cloud of the same run in process; with --mesh (and without
    --cloud: the run builds the cloud for the box all the same) the file holds exactly what fuse extracts and the trajectory is unchanged"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", ["--cloud", str(tmp_path / "plain.ply")]),
                        ("mesh", ["--mesh", str(tmp_path / "surface.ply"), "--mesh-voxel", "0.05", "--mesh-min-weight", "2"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt")] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = r.stdout
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True, keyframe_colour=True)
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_mesh.txt").read_bytes()
    assert (tmp_path / "plain.ply").read_bytes() == CL.ply_bytes(pc.points) and " mesh of " not in said["plain"]
    v, c, t, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True)
    assert (tmp_path / "surface.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0 and c.any()
    assert (f"{info['voxels']} voxels of 0.05 m (truncation 0.2 m), {info['touched']} touched, {v.shape[0]} vertices, {t.shape[0]} triangles"
            in said["mesh"]), said["mesh"]
