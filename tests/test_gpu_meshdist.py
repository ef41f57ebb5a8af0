"""GPU tests of the point-to-mesh distance stage (include/rgbid_meshdist.h, csrc/kernels_meshdist.hip, rgbid.meshdist): the plan's figures and
every output byte for byte against the brute force of tests/meshdist_mirror.py on the cases of tests/test_cpu_meshdist.py, canaries
behind every output; query counts either side of the wave, the compaction tile and the sort tile; queries on cell borders and on, one cell
and two cells outside the grid's outer faces; 32- and 64-bit cell keys; each optional output absent in turn; records against points; the
query sort on and off; plans of every size in every order on one handle and several queries on one plan; every refusal with the handle
used afterwards; the pair-capacity refusal; and the composites: mesh_deviation against the mirror and the command lines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import meshdist as MD
from rgbid import sequence, simplify as SP, smooth as SO, synth, tsdf as TS, tum
from tests import meshdist_mirror as DM
from tests.test_cpu_meshdist import VOXEL, all_cases, case, mirrored, plane_mesh, sphere_mesh, sphere_points
from tests.test_gpu_cloud import K_SMALL, write_tum_folder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
NAN, INF = float("nan"), float("inf")
CAP_V, CAP_T, CAP_P, CAP_Q = 5000, 5000, 200000, 6000
PAD = 3                                                     # rows behind every output that must keep their canary
CANARY = dict(triangle=-7, distance=7.0, closest=-3.0, region=0xA5, candidates=-9)
SHAPES = dict(triangle=((), torch.int32), distance=((), torch.float32), closest=((3,), torch.float32), region=((), torch.uint8),
              candidates=((), torch.int32))


@pytest.fixture(scope="module")
def dist(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh of another size"""
    h = MD.Distance(ctx, CAP_V, CAP_T, CAP_P, CAP_Q)
    yield h
    h.close()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def raw(x):
    return x.cpu().numpy().tobytes()


def records_of(points):
    """rgbid_cloud_point records with the positions of float32 [n, 3] and other bytes elsewhere"""
    rec = np.full((len(points), 8), 0x5A5A5A5A, U32)
    rec[:, :3] = np.ascontiguousarray(points, F).view(U32)
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 32)).cuda()


def assert_planned(dist, m, exp_plan, cell=None):
    got = dist.plan(dev(m["vertices"]), dev(m["triangles"]), m["d_max"], cell)
    assert got["grid"] == exp_plan["grid"].tolist(), (got["grid"], exp_plan["grid"])
    assert {k: got[k] for k in MD.STATS} == {k: exp_plan[k] for k in MD.STATS}, (got, {k: exp_plan[k] for k in MD.STATS})
    return got


def assert_queried(dist, points, exp, outputs=MD.OUTPUTS, records=False):
    """one query into buffers with PAD canary rows behind the n results: every requested output's bytes and every canary"""
    n = len(points)
    out = {k: torch.full((n + PAD,) + SHAPES[k][0], CANARY[k], dtype=SHAPES[k][1], device="cuda") for k in outputs}
    q = records_of(points) if records else dev(np.ascontiguousarray(points, F).reshape(-1, 3))
    dist.ctx.wait_torch_stream()
    dist.query_into(q, records=records, **out)
    dist.ctx.sync()
    for k in outputs:
        assert raw(out[k][:n]) == np.ascontiguousarray(exp[k][:n]).tobytes(), (k, n, out[k][:n].cpu().numpy()[:8], exp[k][:8])
        assert (out[k][n:] == CANARY[k]).all(), k


def expected(m, cell=None):
    r = DM.query(m["vertices"], m["triangles"], m["points"], m["d_max"])
    r["plan"] = DM.plan(m["vertices"], m["triangles"], m["d_max"], cell)
    r["candidates"] = DM.candidates(r["plan"], m["points"])
    return r


# ---- the CPU file's cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_cases_against_the_mirror(dist, name):
    m, exp = all_cases()[name], mirrored(name)
    assert_planned(dist, m, exp["plan"])
    for sort in (True, False):
        dist.sort_queries(sort)
        assert_queried(dist, m["points"], exp)
    assert_queried(dist, m["points"], exp, records=True)


def test_the_cases_reach_the_paths():
    """runs of 1 and of hundreds of triangles, more than 4 096 pairs (a second sort tile), a triangle in thousands of cells"""
    p1, p6, big = mirrored("sphere_1")["plan"], mirrored("sphere_6")["plan"], mirrored("big_triangles")["plan"]
    assert np.diff(p1["starts"]).min() == 1 and p6["longest_run"] >= 200 and p6["pairs"] > 4096 and p1["pairs"] > 4096
    assert big["pairs"] > 40000 and big["participating"] == 2


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_5000():
    v, t = sphere_mesh()
    rng = np.random.default_rng(8)
    q = (sphere_points(5003, seed=6) + rng.normal(0, 0.03, (5003, 3))).astype(F)
    q[::97] = (NAN, 0.5, 0.5)
    q[5::211, 2] = INF
    m = case(v, t, q, VOXEL)
    return m, expected(m)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 4095, 4097, 5003])
def test_query_counts(dist, sphere_5000, n):
    m, exp = sphere_5000
    assert_planned(dist, m, exp["plan"])
    for sort in (True, False):
        dist.sort_queries(sort)
        assert_queried(dist, m["points"][:n], exp)
    dist.sort_queries(True)
    if n == 5003:
        won = exp["triangle"] != DM.NONE
        assert 1000 < won.sum() < 4900 and (exp["candidates"] > 0).sum() > won.sum()


def test_cell_borders_and_outer_faces(dist):
    """queries exactly on cell borders inside the grid, on its outer faces, and one and two cells outside them"""
    v, t = plane_mesh(6, 0.5)
    d_max = 0.5
    cell = float(DM.cell_size(d_max))                                         # 0.53125: the grid is 6 x 6 x 1 cells from 0
    pl = DM.plan(v, t, d_max)
    assert pl["grid"].tolist() == [0, 0, 0, 6, 6, 1]
    ks = np.arange(-2, 9)
    border = np.array([(a * cell, b * cell, c * cell) for a in ks for b in (0, 3, 6, 7, 8) for c in (-2, -1, 0, 1, 2, 3)], F)
    beside = np.concatenate([np.nextafter(border, F(INF)), np.nextafter(border, F(-INF))])
    m = case(v, t, np.concatenate([border, beside]), d_max)
    exp = expected(m)
    assert (exp["candidates"] == 0).sum() > 100 and (exp["triangle"] != DM.NONE).sum() > 50
    assert_planned(dist, m, exp["plan"])
    assert_queried(dist, m["points"], exp)


def test_key_widths(dist):
    """two triangles 40 m apart under 2 cm cells: 6.7e9 cells, 64-bit keys; 1 m apart: 32-bit keys"""
    for far, wide in ((40.0, True), (1.0, False)):
        v = [(0, 0, 0), (0.01, 0, 0), (0, 0.01, 0), (far, far, far), (far + 0.01, far, far), (far, far + 0.01, far)]
        q = [(0.003, 0.003, 0.01), (far + 0.003, far, far - 0.015), (far / 2, far / 2, far / 2), (-0.03, 0, 0), (far + 0.05, far, far)]
        m = case(v, [(0, 1, 2), (3, 4, 5)], q, 0.02)
        exp = expected(m)
        assert (int(np.prod(exp["plan"]["div"].astype(object))) >= 1 << 32) == wide
        assert exp["triangle"].tolist() == [0, 1, DM.NONE, DM.NONE, DM.NONE]
        assert_planned(dist, m, exp["plan"])
        for sort in (True, False):
            dist.sort_queries(sort)
            assert_queried(dist, m["points"], exp)
    dist.sort_queries(True)


def test_a_larger_cell_gives_the_same_results(dist):
    m = all_cases()["regions"]
    exp = expected(m, cell=1.5)
    assert exp["plan"]["pairs"] != mirrored("regions")["plan"]["pairs"] and DM.same(exp, mirrored("regions")) == []
    assert_planned(dist, m, exp["plan"], cell=1.5)
    assert_queried(dist, m["points"], exp)


# ---- handle behaviour -------------------------------------------------------------------------------------------------------------------------
def test_each_optional_output_absent_in_turn(dist):
    m, exp = all_cases()["regions"], mirrored("regions")
    assert_planned(dist, m, exp["plan"])
    for drop in MD.OUTPUTS:
        assert_queried(dist, m["points"], exp, tuple(k for k in MD.OUTPUTS if k != drop))
    for only in MD.OUTPUTS:
        assert_queried(dist, m["points"], exp, (only,))
    got = dist.query(dev(m["points"]))
    assert sorted(got) == ["distance", "triangle"] and raw(got["distance"]) == exp["distance"].tobytes() and raw(got["triangle"]) == exp["triangle"].tobytes()
    got = dist.query_records(records_of(m["points"]), MD.OUTPUTS)
    assert all(raw(got[k]) == exp[k].tobytes() for k in MD.OUTPUTS)


def test_plans_in_every_order_and_queries_on_one_plan(ctx):
    """a handle of the exact capacities of the largest case: a smaller mesh after a larger one and the larger one again, two queries on a plan"""
    names = ["sphere_6", "unit", "big_triangles", "no_triangles", "sphere_6", "nobody_takes_part", "regions", "big_triangles"]
    cap_p = max(mirrored(n)["plan"]["pairs"] for n in names)
    h = MD.Distance(ctx, 2002, 4000, cap_p, 700)
    for name in names:
        m, exp = all_cases()[name], mirrored(name)
        assert_planned(h, m, exp["plan"])
        assert_queried(h, m["points"], exp)
        assert_queried(h, m["points"][::-1], {k: exp[k][::-1] for k in MD.OUTPUTS})
        assert_queried(h, m["points"][:5], exp, ("distance",))
    assert h.timing(True) == dict.fromkeys(MD.STAGES, 0.0)
    m, exp = all_cases()["sphere_2"], mirrored("sphere_2")
    assert_planned(h, m, exp["plan"])
    assert_queried(h, m["points"], exp)
    ms = h.timing(False)
    assert all(ms[k] > 0 for k in MD.STAGES), ms
    h.close()


def test_refusals_and_reuse(dist):
    m, exp = all_cases()["regions"], mirrored("regions")
    v, t, q = dev(m["vertices"]), dev(m["triangles"]), dev(m["points"])
    n_v, n_t, n = v.shape[0], t.shape[0], q.shape[0]
    assert_planned(dist, m, exp["plan"])
    L, h = dist.L, dist._h
    grid, stats = (C.c_longlong * 6)(*([77] * 6)), (C.c_ulonglong * 4)(*([77] * 4))
    plan = lambda nv, pv, nt, pt, d, c: L.rgbid_meshdist_plan(h, C.c_ulonglong(nv), C.c_void_p(pv), C.c_ulonglong(nt), C.c_void_p(pt), C.c_float(d),
                                                               C.c_float(c), grid, stats)
    pv, pt = v.data_ptr(), t.data_ptr()
    bad_plans = [(CAP_V + 1, pv, n_t, pt, 0.75, 0), (n_v, pv, CAP_T + 1, pt, 0.75, 0), (n_v, 0, n_t, pt, 0.75, 0), (n_v, pv, n_t, 0, 0.75, 0),
                 (n_v, pv + 2, n_t, pt, 0.75, 0), (n_v, pv, n_t, pt + 1, 0.75, 0), (0, 0, n_t, pt, 0.75, 0),
                 (n_v, pv, n_t, pt, 0.0, 0), (n_v, pv, n_t, pt, -1.0, 0), (n_v, pv, n_t, pt, NAN, 0), (n_v, pv, n_t, pt, INF, 0),
                 (n_v, pv, n_t, pt, 2.0 ** -61, 0), (n_v, pv, n_t, pt, 2.0 ** 61, 0),
                 (n_v, pv, n_t, pt, 0.75, 0.75), (n_v, pv, n_t, pt, 0.75, -1.0), (n_v, pv, n_t, pt, 0.75, NAN), (n_v, pv, n_t, pt, 0.75, INF),
                 (n_v, pv, n_t, pt, 0.75, 2.0 ** 61)]
    for args in bad_plans:
        assert plan(*args) == -1, args
        assert list(grid) == [77] * 6 and list(stats) == [77] * 4                     # nothing written ...
        assert_queried(dist, m["points"], exp)                                        # ... and the former plan kept
    out = {k: torch.full((n + PAD,) + SHAPES[k][0], CANARY[k], dtype=SHAPES[k][1], device="cuda") for k in MD.OUTPUTS}
    ptrs = [out[k].data_ptr() for k in MD.OUTPUTS]
    query = lambda f, cnt, p, o: f(h, C.c_ulonglong(cnt), C.c_void_p(p), *(C.c_void_p(x) for x in o))
    rec = records_of(m["points"])
    dist.ctx.wait_torch_stream()
    bad = [(L.rgbid_meshdist_query, CAP_Q + 1, q.data_ptr(), ptrs), (L.rgbid_meshdist_query, n, 0, ptrs), (L.rgbid_meshdist_query, n, q.data_ptr() + 2, ptrs),
           (L.rgbid_meshdist_query_records, CAP_Q + 1, rec.data_ptr(), ptrs), (L.rgbid_meshdist_query_records, n, 0, ptrs),
           (L.rgbid_meshdist_query_records, n, rec.data_ptr() + 4, ptrs)]
    for k in (0, 1, 2, 4):                                                            # a misaligned 4-byte output; region is bytes
        bad.append((L.rgbid_meshdist_query, n, q.data_ptr(), ptrs[:k] + [ptrs[k] + 2] + ptrs[k + 1:]))
    for f, cnt, p, o in bad:
        assert query(f, cnt, p, o) == -1
    assert query(L.rgbid_meshdist_query, n, q.data_ptr(), [0] * 5) == 0 and query(L.rgbid_meshdist_query, 0, 0, ptrs) == 0      # nothing to do
    dist.ctx.sync()
    assert all((out[k] == CANARY[k]).all() for k in MD.OUTPUTS)
    assert_queried(dist, m["points"], exp)
    # a bad index: refused after the first launches, the former plan gone, the handle usable
    for where in (0, n_t // 2, n_t - 1):
        tb = m["triangles"].copy()
        tb[where, 1] = n_v
        assert_planned(dist, m, exp["plan"])
        d_tb = dev(tb)
        with pytest.raises(MD._lib.RgbidError):
            dist.plan(v, d_tb, 0.75)
        assert query(L.rgbid_meshdist_query, n, q.data_ptr(), ptrs) == -1             # no plan
    # a box outside the grid's bound
    with pytest.raises(MD._lib.RgbidError):
        dist.plan(dev(np.array([(0, 0, 0), (1e6, 0, 0), (0, 1, 0)], F)), dev(np.array([(0, 1, 2)], U32)), 1.0)
    with pytest.raises(ValueError):
        dist.query(q)
    dist.ctx.sync()
    assert all((out[k] == CANARY[k]).all() for k in MD.OUTPUTS)
    assert_planned(dist, m, exp["plan"])
    assert_queried(dist, m["points"], exp)


def test_pair_capacity_refusal(ctx):
    m, exp = all_cases()["sphere_2"], mirrored("sphere_2")
    need = exp["plan"]["pairs"]
    h = MD.Distance(ctx, 2002, 4000, need - 1, 700)
    small, small_exp = all_cases()["unit"], mirrored("unit")
    assert_planned(h, small, small_exp["plan"])
    with pytest.raises(MD._lib.RgbidError, match=f"needs {need} "):
        h.plan(dev(m["vertices"]), dev(m["triangles"]), m["d_max"])
    assert h.needed_pairs == need and h.planned is None
    with pytest.raises(ValueError):
        h.query(dev(m["points"]))
    assert h.L.rgbid_meshdist_query(h._h, C.c_ulonglong(1), C.c_void_p(dev(m["points"]).data_ptr()), *([C.c_void_p(0)] * 5)) == -1      # the former plan is gone
    assert_planned(h, small, small_exp["plan"])
    assert_queried(h, small["points"], small_exp)
    h.close()
    h = MD.Distance(ctx, 2002, 4000, need, 700)
    assert_planned(h, m, exp["plan"])
    assert_queried(h, m["points"], exp)
    h.close()


# ---- composites ------------------------------------------------------------------------------------------------------------------------------
def mirror_summary(va, ta, points, d_max):
    d = DM.query(va, ta, points, d_max)["distance"]
    return MD.summary(torch.from_numpy(d))


def test_mesh_deviation_against_the_mirror(ctx):
    v, t = sphere_mesh()
    dv, dt = dev(v), dev(t)
    sv, _, st, _, info = SP.simplify_mesh(ctx, dv, None, dt, cell=0.1)
    mv = SO.smooth_mesh(ctx, dv, dt, 5)[0]
    for (bv, bt), d_max in (((sv, st), 0.1), ((mv, dt), 0.05)):
        got = MD.mesh_deviation(ctx, dv, dt, bv, bt, d_max)
        hv, ht = bv.cpu().numpy(), bt.cpu().numpy().view(U32)
        a_to_b, b_to_a = mirror_summary(hv, ht, v, d_max), mirror_summary(v, t, hv, d_max)
        print("sphere against", "its simplification:" if bv is sv else "its smoothing:", got)
        for one, exp in ((got["a_to_b"], a_to_b), (got["b_to_a"], b_to_a)):
            assert one["queries"] == exp["queries"] and one["matched"] == exp["matched"] > 0
            assert all(one[k] == pytest.approx(exp[k], rel=1e-12) for k in ("mean", "rms")) and all(one[k] == exp[k] for k in ("median", "p90", "max"))
        assert got["hausdorff"] == max(a_to_b["max"], b_to_a["max"]) > 0
    rec = records_of(v)
    assert MD.cloud_deviation(ctx, rec, sv, st, 0.1) == MD.mesh_deviation(ctx, dv, dt, sv, st, 0.1)["a_to_b"]
    own = MD.point_deviation(ctx, dv, dv, dt, 0.05)
    assert own["matched"] == 2002 and own["max"] == 0.0


def figures_of(line):
    """the figures of a printed summary line"""
    import re
    m = re.search(r"(\d+) of (\d+) matched, mean (\S+) m, rms (\S+) m, median (\S+) m, 90 % (\S+) m, max (\S+) m", line)
    return m.groups()


def test_track_dataset_options_and_mesh_compare(ctx, tmp_path):
    """without the new options PLY and trajectory are what fuse gives today; --mesh-deviation prints mesh_deviation's figures of the written
    mesh against the extraction, --mesh-reference with the plain run's PLY the same figures once more; the plain run against its own PLY
    is at distance 0 everywhere; mesh_compare.py prints the same for the two files"""
    rows, cols, n = 120, 160, 30                 # the sequence of the other command-line mesh tests: the tool has no keyframe thresholds to set
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    plain = str(tmp_path / "plain.ply")
    said = {}
    for name, extra in (("plain", []), ("simplified", ["--mesh-simplify", "0.08", "--mesh-deviation", "0.16", "--mesh-reference", plain,
                                                       "--mesh-reference-distance", "0.16"]), ("own", ["--mesh-reference", plain])):
        r = subprocess.run(base + ["--out", str(tmp_path / f"traj_{name}.txt"), "--mesh", str(tmp_path / f"{name}.ply"), "--mesh-voxel", "0.04"] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        said[name] = r.stdout
    gs = tum.Dataset(str(root))
    frames = [gs.grab(k, rows, cols) for k in range(len(gs))]
    gs.close()
    depth = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).cuda()
    rgb = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", use_graph=0, keyframe_depth=True, keyframe_colour=True)
    v, c, t, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True)
    sv, sc, st, sinfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, simplify=0.08)
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_simplified.txt").read_bytes() == (tmp_path / "traj_own.txt").read_bytes()
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "own.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0
    assert (tmp_path / "simplified.ply").read_bytes() == TS.mesh_ply_bytes(sv, sc, st)
    assert "mesh deviation" not in said["plain"] and "mesh reference" not in said["plain"]
    got = MD.mesh_deviation(ctx, sv, st, v, t, 0.16)
    lines = {k: [l for l in said["simplified"].splitlines() if k in l] for k in ("mesh deviation:", "mesh reference:")}
    assert len(lines["mesh deviation:"]) == 2 and len(lines["mesh reference:"]) == 2, said["simplified"]
    for k in lines:
        assert MD.summary_line(got["a_to_b"]) in lines[k][0] and MD.summary_line(got["b_to_a"]) in lines[k][1], (lines[k], got)
    assert got["a_to_b"]["matched"] == sv.shape[0] and got["a_to_b"]["max"] > 0
    print("tracked run, simplify 0.08:", got)
    own = [l for l in said["own"].splitlines() if "mesh reference:" in l]
    # every vertex that a triangle names lies on its own mesh, at distance exactly 0; the extraction also writes vertices on the rim of
    # the observed surface that no triangle names, and those have a distance
    named = torch.unique(t.view(-1).to(torch.int64))
    one = MD.Distance(ctx, v.shape[0], t.shape[0], MD.pair_bound(t.shape[0]), v.shape[0])
    one.plan(v, t, 0.16)
    d = one.query(v, ("distance",))["distance"]
    one.close()
    assert named.shape[0] > 0.9 * v.shape[0] and (d[named] == 0).all()
    self_fig = MD.summary(d)
    print("tracked run against itself:", named.shape[0], "of", v.shape[0], "vertices named;", self_fig)
    assert len(own) == 2 and all(MD.summary_line(self_fig) in l for l in own), (own, self_fig)
    assert self_fig["median"] == 0.0 and all(int(figures_of(l)[1]) == v.shape[0] and int(figures_of(l)[0]) >= named.shape[0] for l in own)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mesh_compare.py"), str(tmp_path / "simplified.ply"), plain, "--max-distance", "0.16"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"A -> B: {MD.summary_line(got['a_to_b'])}" in r.stdout and f"B -> A: {MD.summary_line(got['b_to_a'])}" in r.stdout
    assert f"Hausdorff distance, truncated: {got['hausdorff']:.6f} m" in r.stdout
