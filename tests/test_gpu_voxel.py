"""GPU tests of the voxel-grid filter (include/rgbid_voxel.h, csrc/kernels_voxel.hip, rgbid.voxel): the kernels against the numpy
restatement (tests/voxel_mirror.py) byte for byte on synthetic clouds of every shape the sort and the runs must handle, on the engine's
own exports and on a chunked run; the refusals; the --voxel option of tools/track_dataset.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import cloud as CL
from rgbid import sequence, synth, tum
from rgbid import voxel as VX
from tests.test_cpu_cloud import cloud_numpy, make_block, records_equal
from tests.test_cpu_voxel import random_cloud
from tests.test_gpu_cloud import K_SMALL, make_lanes, write_tum_folder
from tests.voxel_mirror import voxel_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def upload(p):
    return torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1, 32).copy()).cuda()


def check(ctx, p, leaf=0.01, min_points=0, dev=None, vg=None):
    """device filter of records p (structured) == the mirror, byte for byte; the plan's counts == the mirror's -> (voxels, plan)"""
    dev = upload(p) if dev is None else dev
    own = vg is None
    vg = VX.VoxelGrid(ctx, max(len(p), 1)) if own else vg
    out, plan = vg.build(dev, leaf, min_points, return_plan=True)
    if own:
        vg.close()
    exp, ep = voxel_numpy(p, leaf, min_points, return_plan=True)
    assert (plan.voxels, plan.finite, plan.runs, plan.kept) == (len(exp), ep["finite"], ep["runs"], ep["kept"])
    if len(exp):
        assert plan.min_b == ep["min_b"] and plan.div_b == ep["div_b"]
    got = VX.as_numpy(out)
    ok, first = records_equal(got, exp)
    assert ok, (first, got[first] if first is not None else None, exp[first] if first is not None else None)
    return got, plan


@pytest.mark.parametrize("n", [0, 1, 17, 4095, 4096, 4097, 3 * 4096 + 1000, (1 << 20) + 3])
def test_voxel_sizes(ctx, n):
    """sizes around the sort's 4 096-key tile and past 2^20, with NaN / inf positions and NaN normals"""
    rng = np.random.default_rng(n)
    p = random_cloud(rng, n, spread=0.2 if n > 4096 else 0.05)
    got, plan = check(ctx, p)
    if n >= 4096:
        assert plan.finite < n and 1 < len(got) < plan.finite


def test_voxel_min_points_and_anisotropic_leaf(ctx):
    rng = np.random.default_rng(11)
    p = random_cloud(rng, 200_000, spread=0.1)
    for leaf, minp in (((0.01, 0.02, 0.005), 0), (0.02, 5), (0.005, 2), (0.05, 1_000_000)):
        check(ctx, p, leaf, minp)


def test_voxel_every_point_its_own_voxel(ctx):
    """cell centres of a 1 cm grid, shuffled: as many voxels as points, in key order"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(np.arange(61), np.arange(53), np.arange(47), indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    p = random_cloud(rng, len(g), nan=0.0)
    for a, c in enumerate("xyz"):
        p[c] = ((g[:, a] + 0.5) * 0.01 - 0.2).astype(np.float32)
    got, plan = check(ctx, p)
    assert len(got) == len(p) and (got["count"] == 1).all()


def test_voxel_one_voxel_of_a_million(ctx):
    rng = np.random.default_rng(4)
    n = 1 << 20
    p = random_cloud(rng, n, nan=0.0)
    for c in "xyz":
        p[c] = rng.uniform(0.3001, 0.3099, n).astype(np.float32)
    got, plan = check(ctx, p)
    assert len(got) == 1 and got["count"][0] == n


def test_voxel_64bit_keys(ctx):
    """a key space of ~2^60 cells: the 64-bit key path (8 radix passes); cells shared by 1 - 3 points"""
    rng = np.random.default_rng(5)
    n = 300_000
    cells = rng.integers(0, 1 << 20, (n // 2, 3))
    cells = np.concatenate([cells, cells[rng.integers(0, len(cells), n - len(cells))]])
    cells = cells[rng.permutation(n)]
    p = random_cloud(rng, n, nan=0.01)
    for a, c in enumerate("xyz"):
        p[c] = np.where(np.isfinite(p[c]), (cells[:, a] + rng.uniform(0.1, 0.9, n)).astype(np.float32), p[c])
    got, plan = check(ctx, p, leaf=1.0)
    cells_total = plan.div_b[0] * plan.div_b[1] * plan.div_b[2]
    assert cells_total > 1 << 32 and len(got) < plan.finite


def test_voxel_non_finite_inputs(ctx):
    rng = np.random.default_rng(6)
    p = random_cloud(rng, 50_000, nan=0.3)
    p["y"][rng.random(len(p)) < 0.1] = -np.inf
    check(ctx, p)
    q = p.copy()
    q["x"] = np.nan
    got, plan = check(ctx, q)
    assert len(got) == 0 and plan.finite == 0


def test_voxel_offset_inputs_and_reuse(ctx):
    """records starting 1 and 3 records into a buffer, odd counts; one filter reused across plans of different sizes"""
    rng = np.random.default_rng(7)
    p = random_cloud(rng, 30_011, spread=0.1)
    dev = upload(p)
    vg = VX.VoxelGrid(ctx, len(p))
    for off, end, leaf, minp in ((1, len(p), 0.01, 0), (3, 20_000, (0.02, 0.01, 0.01), 2), (0, 5, 0.01, 0), (0, len(p), 0.03, 3)):
        check(ctx, p[off:end], leaf, minp, dev=dev[off:end], vg=vg)
    vg.close()


def test_voxel_deterministic(ctx):
    rng = np.random.default_rng(8)
    p = random_cloud(rng, 1 << 20, spread=0.3)
    dev = upload(p)
    a = VX.voxel_grid(ctx, dev, 0.01)
    b = VX.voxel_grid(ctx, dev, 0.01)
    assert torch.equal(a, b) and len(a) > 0


def test_voxel_refusals(ctx):
    rng = np.random.default_rng(9)
    p = random_cloud(rng, 100, nan=0.0)
    dev = upload(p)
    vg = VX.VoxelGrid(ctx, 100)
    for leaf in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            vg.plan(dev, leaf)
    L = vg.L
    nv = C.c_ulonglong()
    for leaf in ((0.0, 0.01, 0.01), (0.01, float("inf"), 0.01), (0.01, 0.01, -0.01)):    # the C-ABI itself, past the Python check
        assert L.rgbid_voxel_plan(vg._h, C.c_void_p(dev.data_ptr()), 100, (C.c_float * 3)(*leaf), 0, None, None, C.byref(nv)) == -1
    lf = (C.c_float * 3)(0.01, 0.01, 0.01)
    assert L.rgbid_voxel_plan(vg._h, C.c_void_p(dev.data_ptr()), 101, lf, 0, None, None, C.byref(nv)) == -1       # n > max_points
    assert L.rgbid_voxel_plan(vg._h, C.c_void_p(dev.data_ptr() + 8), 50, lf, 0, None, None, C.byref(nv)) == -1    # not 16-byte aligned
    assert L.rgbid_voxel_plan(vg._h, None, 5, lf, 0, None, None, C.byref(nv)) == -1
    far = p.copy(); far["x"][0] = 3e7                                                   # floor(3e7 / 0.01) is outside int32
    with pytest.raises(Exception):
        vg.plan(upload(far), 0.01)
    big = p.copy()
    for c in "xyz":
        big[c][0], big[c][1] = 0.0, 2.0 ** 21 - 1                                       # 2^63 cells
    with pytest.raises(Exception):
        vg.plan(upload(big), 1.0)
    plan = vg.plan(dev, 0.01)                                                           # the filter still works after a refusal
    assert plan.voxels > 0
    with pytest.raises(Exception):
        vg.emit(torch.empty((plan.voxels - 1, 32), dtype=torch.uint8, device="cuda"))   # capacity below the plan's voxels
    vg.close()


def test_voxel_from_engine_exports(ctx):
    """engine exports -> Cloud.build -> VoxelGrid.build, against the mirror applied to the restated cloud"""
    rows, cols, n, B = 120, 160, 9, 2
    from rgbid import engine as E
    seqs, depth, rgb = make_lanes(B, n, rows, cols, K_SMALL, trans_step=(0.01, 0.02), rot_step_deg=(0.5, 1.0))
    eng = E.Engine(ctx, E.default_config(rows=rows, cols=cols, lanes=B, K=K_SMALL, record_capacity=n, keyframe_capacity=8,
                                         visratio_odo=0.985, visratio_integr=0.97))
    for k in range(n):
        eng.step(depth[k], rgb[k])
    counts = eng.keyframe_counts()
    pairs = [(l, s) for l in range(B) for s in range(int(counts[l]))]
    srcs, _ = eng.keyframe_sources(pairs)
    kfs = [eng.read_keyframe(l, s) for l, s in pairs]
    cl = CL.Cloud(ctx, rows, cols, len(pairs))
    for mode in ("all", "novel"):
        pts, _ = cl.build(srcs, K_SMALL, mode)
        raw = np.concatenate([cloud_numpy(make_block(a["overlap_mask"], a["colors"], a["depthinv"], a["normals"]), rows, cols, K_SMALL, a["R"],
                                          a["t"], mode) for a in kfs])
        assert records_equal(CL.as_numpy(pts), raw)[0]
        got, plan = check(ctx, raw, 0.01, dev=pts)
        assert 0 < len(got) < len(raw)
    cl.close(); eng.close()


def test_voxel_chunked_cloud_against_the_scene(ctx):
    """the 2-chunk noise-free run of test_chunked_cloud_against_the_scene: every centroid lies in its own cell's closed box, and the
    centroids stay on the scene's height field within the raw cloud's bound plus leaf / 2"""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    R, t, ranges, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97)
    leaf = 0.01
    vox, plan = VX.voxel_grid(ctx, pc.points, leaf, return_plan=True)
    v = VX.as_numpy(vox)
    raw = pc.numpy()
    exp = voxel_numpy(raw, leaf)
    assert records_equal(v, exp)[0]
    assert 0 < len(v) < len(raw) and int(v["count"].sum()) == plan.finite
    # each voxel's cell from its members' keys (ascending key order = the voxel order)
    fin = np.isfinite(raw["x"]) & np.isfinite(raw["y"]) & np.isfinite(raw["z"])
    inv = np.float32(1) / np.float32(leaf)
    ijk = [(np.floor(raw[c][fin] * inv) - np.float32(plan.min_b[a])).astype(np.int64) for a, c in enumerate("xyz")]
    keys = np.unique(ijk[0] + ijk[1] * plan.div_b[0] + ijk[2] * plan.div_b[0] * plan.div_b[1])
    assert len(keys) == len(v)
    cell = [keys % plan.div_b[0], (keys // plan.div_b[0]) % plan.div_b[1], keys // (plan.div_b[0] * plan.div_b[1])]
    for a, c in enumerate("xyz"):
        lo = (cell[a] + plan.min_b[a]) * np.float64(leaf)
        assert (v[c] >= lo - 1e-6).all() and (v[c] <= lo + leaf + 1e-6).all(), c
    scene = synth.Scene(seed=synth.SEED)
    xyz = torch.from_numpy(np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float64))
    res = np.abs((xyz[:, 2] - scene.depth(xyz[:, 0], xyz[:, 1])).numpy())
    med = float(np.median(res[np.isfinite(res)]))
    print(f"voxels vs scene: {len(v)} voxels of {plan.finite} points, median |z - f(x, y)| {med * 1e3:.3f} mm")
    assert med <= 1.5e-3 + leaf / 2, med


def _ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    nv = int([l for l in head.split(b"\n") if l.startswith(b"element vertex")][0].split()[-1])
    assert len(body) == 27 * nv
    return data, nv, body


def test_track_dataset_voxel_option(ctx, tmp_path):
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    runs = {}
    for name, extra in (("cloud", ["--cloud", str(tmp_path / "raw.ply")]), ("voxel", ["--cloud", str(tmp_path / "vox.ply"), "--voxel", "0.01"])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt")] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = r.stdout
    assert (tmp_path / "traj_cloud.txt").read_bytes() == (tmp_path / "traj_voxel.txt").read_bytes()
    raw, nraw, body = _ply(tmp_path / "raw.ply")
    vox, nvox, _ = _ply(tmp_path / "vox.ply")
    assert 0 < nvox < nraw
    assert f"{nraw} points" in runs["voxel"] and f"{nvox} voxels" in runs["voxel"], runs["voxel"]
    # --cloud alone is what it was: the raw cloud of the same run in process
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0)
    assert CL.ply_bytes(pc.points) == raw
    vg, plan = VX.voxel_grid(ctx, pc.points, 0.01, return_plan=True)
    assert plan.voxels == nvox and CL.ply_bytes(vg) == vox
