"""GPU tests of the alignment of depth frames to the TSDF volume (include/rgbid_tsdf_align.h, csrc/kernels_tsdf.hip, rgbid.tsdf): the bytes of
the result records -- poses, status, iterations, used counts and both sets of 28 sums -- against the numpy restatement
(tests/align_mirror.py) on the prototype scene with whole and ragged lattices at every stride, several levels, a Huber threshold below trunc
and damping; lattices of 300 and 4 800 tiles; the threshold scene to the ulp; views that converge, run, are FEW and are SINGULAR in one call;
a plan that survives an alignment; a smaller volume after a larger one; the refusals; a tracked run and the option of
tools/track_dataset.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import sequence, synth, tsdf as TS, tum
from tests import align_mirror as AM
from tests import tsdf_mirror as TM
from tests.test_cpu_align import TH_ALIGN_CASES, exact_planes, perturbed, proto_scene, th_align
from tests.test_cpu_consist import COLS, K, ROWS
from tests.test_cpu_tsdf import GATE, TH_K
from tests.test_gpu_cloud import K_SMALL, write_tum_folder
from tests.test_gpu_raycast import loaded
from tests.test_gpu_tsdf import mirror_of_fuse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DEFAULTS = dict(levels=TS.ALIGN_LEVELS, huber=None, damping=0.0, eps=1e-6, min_pixels=64, min_weight=1, z_min=0.05, z_max=20.0)


def device_records(ctx, vol, planes, R, t, K_, rows, cols, **kw):
    """Volume.align_into's records as a numpy array of ALIGN_RESULT, with canaries before and behind them"""
    a = dict(DEFAULTS, **kw)
    V = len(np.asarray(R).reshape(-1, 3, 3))
    n = V * TS.ALIGN_RESULT.itemsize
    buf = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(planes), F)).cuda()
    ctx.wait_torch_stream()
    vol.align_into(dev, R, t, K_, rows, cols, a["levels"], a["huber"], a["damping"], a["eps"], a["min_pixels"], a["min_weight"], a["z_min"],
                   a["z_max"], buf[16:16 + n])
    ctx.sync()
    assert (buf[:16] == 0xA5).all() and (buf[16 + n:] == 0xA5).all()
    return buf[16:16 + n].cpu().numpy().view(TS.ALIGN_RESULT)


def assert_align(ctx, vol, mirror, planes, R, t, K_, rows, cols, **kw):
    """-> the mirror's records, which the device's equal byte for byte"""
    a = dict(DEFAULTS, **kw)
    got = device_records(ctx, vol, planes, R, t, K_, rows, cols, **kw)
    want = AM.align(mirror, planes, R, t, K_, rows, cols, **a)
    for name in ("status", "iterations", "used"):
        assert np.array_equal(got[name], want[name]), (name, got[name].tolist(), want[name].tolist())
    for name in ("sums", "pose"):
        g, e = got[name].view(np.uint64), want[name].view(np.uint64)
        bad = np.nonzero(g != e)
        assert bad[0].size == 0, (name, bad[0].size, [b[:5] for b in bad], got[name][bad][:5], want[name][bad][:5])
    assert got.tobytes() == want.tobytes()
    return want


@pytest.mark.parametrize("V", [1, 3, 17])
def test_align_prototype_scene_shapes(ctx, V):
    vol = None
    for rows, cols in ((ROWS, COLS), (ROWS - 1, COLS - 1)):          # whole 8 x 8 tiles at stride 1, and ragged ones
        sc = proto_scene(V, rows, cols)
        vol = loaded(ctx, sc["vol"], vol=vol)
        Rp, tp = perturbed(sc["R"], sc["t"], 0.02, 0.03, 40 + V)
        for stride in (1, 2, 4, 8):                                   # 8: a lattice of 6 x 8, one ragged tile
            want = assert_align(ctx, vol, sc["vol"], sc["planes"], Rp, tp, K, rows, cols, levels=((stride, 3),), min_pixels=6, **GATE)
            assert (want["iterations"] == 3).all() and (want["used"][:, 0] >= 30).all(), (stride, want["used"][:, 0])
        want = assert_align(ctx, vol, sc["vol"], sc["planes"], Rp, tp, K, rows, cols, levels=((4, 3), (2, 3), (1, 4)), huber=0.02, damping=1e-3,
                            eps=1e-4, **GATE)
        assert (want["iterations"] >= 3).all() and (want["sums"][:, 1, 27] < want["sums"][:, 0, 27]).all()
    vol.close()


@pytest.mark.parametrize("scale,iterations,tiles", [(2.5, 4, 300), (10.0, 2, 4800)])
def test_align_large_lattices(ctx, scale, iterations, tiles):
    """one view of 120 x 160 (300 tiles: two rounds of the upper tree) and one of 480 x 640 (4 800 tiles: three rounds)"""
    sc = proto_scene()
    rows, cols = int(ROWS * scale), int(COLS * scale)
    Kl = (K[0] * scale, K[1] * scale, (K[2] + 0.5) * scale - 0.5, (K[3] + 0.5) * scale - 0.5)
    assert ((rows + 7) // 8) * ((cols + 7) // 8) == tiles
    planes = exact_planes(sc["R"][1:2], sc["t"][1:2], rows, cols, Kl)
    planes[0, ::7, ::5] = np.nan
    Rp, tp = perturbed(sc["R"][1:2], sc["t"][1:2], 0.02, 0.03, 3)
    vol = loaded(ctx, sc["vol"])
    want = assert_align(ctx, vol, sc["vol"], planes, Rp, tp, Kl, rows, cols, levels=((1, iterations),), **GATE)
    assert want["iterations"][0] == iterations and want["used"][0, 0] > 0.7 * rows * cols
    vol.close()


def test_align_thresholds_to_the_ulp(ctx):
    """every view of every case of the threshold scene alone (tests/test_cpu_align.py asserts what each of them is about), then a case's
    views in one call"""
    vol = None
    for name, c in TH_ALIGN_CASES.items():
        n = len(c["views"])
        for sel in [[v] for v in range(n)] + ([list(range(n))] if n > 1 else []):
            mirror, planes, R, t, a = th_align(name, sel)
            vol = loaded(ctx, mirror, vol=vol)
            assert_align(ctx, vol, mirror, planes, R, t, TH_K, ROWS, COLS, **a)
    vol.close()


@functools.lru_cache(maxsize=None)
def status_scene():
    """the prototype volume with a block of constant D = 0.05 at its +x end (no gradient: H = 0 exactly), and five views: 0 at its true
    pose, 1 with all but 40 pixels unmeasured (FEW under min_pixels = 64), 2 that sees the block only (SINGULAR), 3 and 4 perturbed.
    Under eps = 0.01 and the levels (2, 4), (1, 4) the mirror has views 0 and 4 meet eps before a level's end (6 systems instead of
    8), view 4 ending CONVERGED and view 0 RUNNING, and view 3 use all 8"""
    sc = proto_scene()
    vol = TM.Volume(sc["vol"].nx, sc["vol"].ny, sc["vol"].nz, sc["vol"].origin, sc["vol"].voxel, sc["vol"].trunc)
    D, W = sc["vol"].D.copy(), sc["vol"].W.copy()
    D[:, :, 48:], W[:, :, 48:] = F(0.05), 1
    vol.set_state(D, W)
    Rp, tp = perturbed(sc["R"], sc["t"], 0.03, 0.04, 9)
    R = np.stack([sc["R"][0], sc["R"][1], np.eye(3), Rp[3], Rp[4]])
    t = np.stack([sc["t"][0], sc["t"][1], [1.2, 0.0, 0.0], tp[3], tp[4]])
    planes = sc["planes"][[0, 1, 2, 3, 4]].copy()
    few = np.full((ROWS, COLS), np.nan, F)
    few[20:25, 30:38] = planes[1][20:25, 30:38]
    planes[1] = few
    block = np.full((ROWS, COLS), np.nan, F)
    block[16:32, 24:40] = F(1 / 1.8)                        # |x - 1.2| < 0.25, |y| < 0.25 at z = 1.8: inside the block
    planes[2] = block
    return vol, planes, R, t


def test_align_views_that_stop_beside_views_that_run(ctx):
    mirror, planes, R, t = status_scene()
    vol = loaded(ctx, mirror)
    want = assert_align(ctx, vol, mirror, planes, R, t, K, ROWS, COLS, levels=((2, 4), (1, 4)), eps=0.01, **GATE)
    print("status", want["status"], "iterations", want["iterations"], "used", want["used"].tolist())
    assert want["status"][1] == AM.FEW and want["iterations"][1] == 1 and 0 < want["used"][1, 0] < 64
    assert want["status"][2] == AM.SINGULAR and want["iterations"][2] == 1 and want["used"][2, 0] >= 64 and not want["sums"][2, 0, :27].any()
    assert want["iterations"][0] < 8 and want["iterations"][4] < 8 and want["iterations"][3] == 8      # two stopped early in a level
    assert set(want["status"]) == {AM.RUNNING, AM.CONVERGED, AM.FEW, AM.SINGULAR}
    for v in (1, 2):                                        # the pose stays as it was given
        assert want["pose"][v].tobytes() == np.concatenate([R[v].reshape(9), t[v]]).tobytes()
    vol.close()


def test_plan_survives_an_alignment_and_a_smaller_volume_follows_a_larger(ctx):
    sc = proto_scene()
    mirror = sc["vol"]
    vol = loaded(ctx, mirror, max_views=8)
    ev, ec, et = TM.extract(mirror, 1)
    nv, nt = C.c_ulonglong(), C.c_ulonglong()
    ctx.wait_torch_stream()
    assert vol.L.rgbid_tsdf_extract_plan(vol._h, 1, C.byref(nv), C.byref(nt)) == 0 and (nv.value, nt.value) == (len(ev), len(et))
    Rp, tp = perturbed(sc["R"], sc["t"], 0.02, 0.03, 5)
    before = [x.clone() for x in vol.state()]
    assert_align(ctx, vol, mirror, sc["planes"], Rp, tp, K, ROWS, COLS, levels=((2, 2), (1, 2)), **GATE)      # reads the state only
    for a, b in zip(before, vol.state()):
        assert torch.equal(a, b)
    verts = torch.empty((len(ev), 3), dtype=torch.float32, device="cuda")
    tris = torch.empty((len(et), 3), dtype=torch.int32, device="cuda")
    ctx.wait_torch_stream()
    vol.emit(verts, None, tris)
    ctx.sync()
    assert verts.cpu().numpy().tobytes() == ev.tobytes() and tris.cpu().numpy().view(np.uint32).tobytes() == et.tobytes() and len(et) > 1000
    # a smaller volume on the same handle: the middle of the larger one, and a smaller image (the workspace was sized by the larger call)
    small = TM.Volume(40, 30, 20, (-1.0, -0.75, 1.3), 0.05, 0.2)
    small.set_state(mirror.D[6:26, 9:39, 12:52], mirror.counts()[6:26, 9:39, 12:52])
    loaded(ctx, small, vol=vol)
    want = assert_align(ctx, vol, small, sc["planes"][:, :40, :50], Rp, tp, K, 40, 50, levels=((1, 3),), **GATE)
    assert (want["used"][:, 0] > 200).all()
    vol.close()


def test_align_refusals_and_reuse(ctx):
    sc = proto_scene()
    mirror = sc["vol"]
    vol = loaded(ctx, mirror, max_views=3)
    L = vol.L
    R, t = sc["R"][:3], sc["t"][:3]
    planes = torch.from_numpy(np.ascontiguousarray(sc["planes"][:3])).cuda()
    n = 3 * TS.ALIGN_RESULT.itemsize
    result = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")

    def view_table(R_=R, t_=t, V=3, off=0, null=False):
        return (TS.View * V)(*[TS.View(TS.Pose((C.c_double * 9)(*np.asarray(R_[v], np.float64).reshape(9)), (C.c_double * 3)(*t_[v])),
                                       None if null and v == 1 else planes[v].data_ptr() + (off if v == 2 else 0), None) for v in range(V)])

    def levels_of(lv):
        return (C.c_int * (2 * len(lv)))(*[x for l in lv for x in l])

    def call(V=3, views=None, K_=K, rows=ROWS, cols=COLS, z_min=0.3, z_max=5.0, mw=1, huber=0.2, damping=0.0, eps=1e-6, mp=64, lv=((2, 2), (1, 2)),
             n_levels=None, r=8):
        ctx.wait_torch_stream()
        return L.rgbid_tsdf_align(vol._h, V, view_table() if views is None else views, (C.c_float * 4)(*K_), rows, cols, z_min, z_max, mw, huber,
                                  damping, eps, mp, len(lv) if n_levels is None else n_levels, levels_of(lv) if lv else None,
                                  result.data_ptr() + r if r is not None else None)

    nan, inf = float("nan"), float("inf")
    Rn = R.copy(); Rn[1, 0, 0] = nan
    ti = t.copy(); ti[2, 1] = inf
    tb = t.copy(); tb[0, 0] = 1e39                          # finite as double, infinite as float32
    refusals = [lambda: call(V=0), lambda: call(V=4), lambda: call(V=-1), lambda: call(rows=0), lambda: call(cols=0), lambda: call(rows=-3),
                lambda: call(cols=(1 << 20) + 1), lambda: call(rows=1 << 15, cols=1 << 15),
                lambda: call(z_min=0.0), lambda: call(z_min=-1.0), lambda: call(z_min=nan), lambda: call(z_max=nan), lambda: call(z_max=inf),
                lambda: call(z_min=2.0, z_max=1.0), lambda: call(mw=0), lambda: call(mw=65536),
                lambda: call(huber=0.0), lambda: call(huber=-0.1), lambda: call(huber=nan), lambda: call(huber=inf),
                lambda: call(damping=-1e-9), lambda: call(damping=nan), lambda: call(damping=inf),
                lambda: call(eps=0.0), lambda: call(eps=-1.0), lambda: call(eps=nan), lambda: call(eps=inf), lambda: call(mp=5), lambda: call(mp=0),
                lambda: call(lv=((1, 1),), n_levels=0), lambda: call(lv=((1, 1),) * 5), lambda: call(lv=((3, 1),)), lambda: call(lv=((0, 1),)),
                lambda: call(lv=((16, 1),)), lambda: call(lv=((1, 0),)), lambda: call(lv=((1, -2),)), lambda: call(lv=((1, 257),)),
                lambda: call(lv=((1, 128), (2, 129))), lambda: call(lv=None, n_levels=1),
                lambda: call(views=view_table(R_=Rn)), lambda: call(views=view_table(t_=ti)), lambda: call(views=view_table(t_=tb)),
                lambda: call(K_=(nan, 58.0, 31.5, 23.5)), lambda: call(K_=(60.0, 58.0, inf, 23.5)), lambda: call(K_=(0.0, 58.0, 31.5, 23.5)),
                lambda: call(K_=(60.0, 0.0, 31.5, 23.5)), lambda: call(views=view_table(off=2)), lambda: call(views=view_table(null=True)),
                lambda: call(r=None), lambda: call(r=4), lambda: call(r=9)]

    Rp, tp = perturbed(R, t, 0.02, 0.03, 6)

    def still_works():
        assert_align(ctx, vol, mirror, sc["planes"][:3, :ROWS - 1, :COLS - 1], Rp, tp, K, ROWS - 1, COLS - 1, levels=((2, 2), (1, 2)), **GATE)

    still_works()
    before = [x.clone() for x in vol.state()]
    for i, r in enumerate(refusals):
        assert r() == -1, i
    ctx.sync()
    assert (result == 0xA5).all()                           # the result is untouched
    for a, b in zip(before, vol.state()):
        assert torch.equal(a, b)
    still_works()
    for i in (0, 8, 16, 23, 31, 39, 46, 49):                # the handle is usable after each kind of refusal, not only after all
        assert refusals[i]() == -1, i
        still_works()
    assert call() == 0                                      # the same call with nothing wrong
    ctx.sync()
    want = AM.align(mirror, sc["planes"][:3], R, t, K, ROWS, COLS, ((2, 2), (1, 2)), huber=0.2, **GATE)
    assert result[8:8 + n].cpu().numpy().tobytes() == want.tobytes() and (result[:8] == 0xA5).all() and (result[8 + n:] == 0xA5).all()
    for bad in (dict(z_min=0), dict(R=Rn), dict(K=(0, 1, 1, 1)), dict(rows=0), dict(huber=0.0), dict(min_weight=0), dict(levels=((3, 1),)),
                dict(min_pixels=5), dict(eps=0), dict(damping=-1), dict(R=np.stack([np.eye(3)] * 4), t=np.zeros((4, 3)))):
        a = dict(planes=planes, R=R, t=t, K=K, rows=ROWS, cols=COLS)
        a.update(bad)
        with pytest.raises(ValueError):                    # the Python checks come first
            vol.align(**a)
    vol.timing(True)
    still_works()
    ms = vol.align_timing(False)
    print("tsdf align ms:", ms)
    assert set(ms) == set(TS.ALIGN_STAGES) and all(np.isfinite(x) and x > 0 for x in ms.values())
    d = vol.align(planes, Rp, tp, K, ROWS, COLS, ((2, 2), (1, 2)), **GATE)                                 # the dict is the records
    m = AM.as_dict(AM.align(mirror, sc["planes"][:3], Rp, tp, K, ROWS, COLS, ((2, 2), (1, 2)), **GATE))
    assert set(d) == set(m) and all(d[k].tobytes() == m[k].tobytes() for k in m)
    vol.close()


# ---- a tracked run and the command line -----------------------------------------------------------------------------------------------
def _figures_line(figures):
    run = TS.align_check_summary(figures)
    return (f"mesh align check: {run['views']} keyframes aligned to the model of the others: correction median "
            f"{run['rotation_median']:.6f} rad {run['translation_median']:.6f} m, largest {run['rotation_max']:.6f} rad {run['translation_max']:.6f} m; "
            + ", ".join(f"{n} {w}" for w, n in run["status"].items()))


def test_align_check_on_a_tracked_run(ctx):
    """the tracked run of tests/test_gpu_tsdf.py (2 chunks, 160 x 120, voxel 0.04 m): the odd keyframes aligned to the model of the even
    ones equal the mirror's bytes.  The corrections are printed, not asserted."""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                         keyframe_colour=True)
    kfs = pc.keyframes
    assert len(kfs) >= 3
    levels = ((4, 3), (2, 3), (1, 3))
    figures, got = TS.align_check(ctx, kfs, K_SMALL, rows, cols, voxel=0.04, points=pc.points, levels=levels, return_results=True)
    print("tracked run:", _figures_line(figures))
    for f in figures:
        print(f)
    even, odd = kfs[0::2], kfs[1::2]
    assert [f["keyframe"] for f in figures] == list(range(1, len(kfs), 2)) and len(figures) == len(odd)
    *_, info, vol = TS.fuse(ctx, even, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, keep_volume=True)
    vol.close()

    class Even:
        keyframes = even
    mirror = mirror_of_fuse(Even, info, 0.04, 0.16, K_SMALL)
    want = AM.as_dict(AM.align(mirror, [k["depthinv"].cpu().numpy() for k in odd], np.stack([k["R"] for k in odd]), np.stack([k["t"] for k in odd]),
                               K_SMALL, rows, cols, levels))
    assert set(got) == set(want) and all(got[k].tobytes() == want[k].tobytes() for k in want), [k for k in want if got[k].tobytes() != want[k].tobytes()]
    assert (want["used"][:, 0] > 1000).all()


def test_track_dataset_mesh_align_check(ctx, tmp_path):
    """--mesh without the option writes what it wrote and says nothing of an alignment; with it the files are the same bytes and the
    printed numbers are align_check's"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("new", ["--mesh-align-check", "--mesh-align-iterations", "3"])):
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
    v, c, t = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, points=pc.points)
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_new.txt").read_bytes()
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "new.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0
    assert "mesh align check" not in said["plain"]
    figures = TS.align_check(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, points=pc.points, levels=((4, 3), (2, 3), (1, 3)))
    assert "rank 0: " + _figures_line(figures) in said["new"], said["new"][-1500:]
