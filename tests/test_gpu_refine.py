"""GPU tests of the edge split (include/rgbid_refine.h, csrc/kernels_refine.hip, rgbid.refine): the nine counts and the emitted vertices,
colours, normals, triangles and selection byte for byte against the numpy restatement (tests/refine_mirror.py) on the meshes of
tests/test_cpu_refine.py, with and without each attribute, canaries behind every output; triangle counts either side of a block and of
the tiles; edge and marked-edge counts either side of the tiles; vertex counts either side of a change in the sort's pass count; a hub
of 1 024 triangles and an edge in 64; random soups with every pattern; plans and emits in every order on one handle of exact capacities;
every refusal; the one-shot's rounds; and the options of rgbid.tsdf and tools/track_dataset.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import refine as RF, sequence, synth, tsdf as TS, tum
from tests import holes_mirror as HM
from tests import refine_mirror as RM
from tests import tsdf_mirror as TM
from tests.test_cpu_holes import attributes, mesh
from tests.test_cpu_refine import all_cases, emitted, median_edge, planned, random_soup, refined
from tests.test_gpu_cloud import K_SMALL, write_tum_folder
from tests.test_gpu_denoise import mirrored as mirrored_denoise
from tests.test_gpu_smooth import RUN_TILE, SORT_TILE, dev, full, raw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32, U8 = np.float32, np.uint32, np.uint8
CAP_V, CAP_T = 70001, 21001
PAD = 3                                                     # rows behind every output that must keep their canary


@pytest.fixture(scope="module")
def rf(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh of another size"""
    h = RF.Refiner(ctx, CAP_V, CAP_T)
    yield h
    h.close()


def with_attributes(m):
    if m.get("colours") is None:
        c, n = attributes(len(m["vertices"]), len(m["triangles"]))
        m = dict(m, colours=c, normals=n)
    return m


def assert_emitted(rf, m, exp, colours=True, normals=True, selection=True):
    """one emit into buffers of exactly the rows of the result with PAD canary rows behind them: the bytes, the canaries, the inputs untouched"""
    ev, ec, en, et, es = exp
    n_t = len(m["triangles"])
    sel = (np.ones(n_t, U8) if m["selection"] is None else m["selection"]) if selection else None
    ins = [dev(m["vertices"]), dev(m["colours"]) if colours else None, dev(m["normals"]) if normals else None, dev(m["triangles"]),
           None if sel is None else dev(sel)]
    before = [None if x is None else raw(x) for x in ins]
    rows_v, rows_t = len(ev), len(et)
    outs = [full(rows_v, (3,), torch.float32, 7.0), full(rows_v, (3,), torch.uint8, 0xA5) if colours else None,
            full(rows_v, (3,), torch.float32, -3.0) if normals else None, full(rows_t, (3,), torch.int32, -9),
            full(rows_t, (), torch.uint8, 0x5A) if selection else None]
    cut = lambda x, rows: None if x is None else x[:rows]
    rf.ctx.wait_torch_stream()
    rf.emit_into(*ins, cut(outs[0], rows_v), cut(outs[1], rows_v), cut(outs[2], rows_v), cut(outs[3], rows_t), cut(outs[4], rows_t))
    rf.ctx.sync()
    got_v, got_t = outs[0][:rows_v].cpu().numpy(), outs[3][:rows_t].cpu().numpy().view(U32)
    assert got_t.tobytes() == et.tobytes(), np.nonzero((got_t != et).any(1))[0][:10]
    assert got_v.tobytes() == ev.tobytes(), np.nonzero((got_v.view(U32) != ev.view(U32)).any(1))[0][:10]
    assert (outs[0][rows_v:] == 7.0).all() and (outs[3][rows_t:] == -9).all()
    if colours:
        assert raw(outs[1][:rows_v]) == ec.tobytes() and (outs[1][rows_v:] == 0xA5).all()
    if normals:
        assert raw(outs[2][:rows_v]) == en.tobytes() and (outs[2][rows_v:] == -3.0).all()
    if selection:
        assert raw(outs[4][:rows_t]) == es.tobytes() and (outs[4][rows_t:] == 0x5A).all()
    assert [None if x is None else raw(x) for x in ins] == before


def assert_planned(rf, m, table):
    got = rf.plan(dev(m["triangles"]), dev(m["vertices"]), m["max_edge"], None if m["selection"] is None else dev(m["selection"]))
    assert got == table["counts"], (got, table["counts"])


def assert_round(rf, m, variants=((True, True, True),)):
    """a mesh that is no case of the CPU file: the plan and emits against the mirror -> the mirror's counts"""
    m = with_attributes(m)
    table = RM.plan(m["triangles"], m["vertices"], m["max_edge"], m["selection"])
    assert_planned(rf, m, table)
    sel = np.ones(len(m["triangles"]), U8) if m["selection"] is None else m["selection"]
    exp = RM.emit(table, m["vertices"], m["colours"], m["normals"], sel)
    for colours, normals, selection in variants:
        assert_emitted(rf, m, exp, colours, normals, selection)
    return table["counts"]


def case(m, max_edge, selection=None):
    return dict(m, selection=None if selection is None else np.ascontiguousarray(selection, U8), max_edge=float(max_edge))


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_cases_against_the_mirror(rf, name):
    m = all_cases()[name]
    assert_planned(rf, m, planned(name))
    exp = emitted(name)
    for colours, normals, selection in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        assert_emitted(rf, m, exp, colours, normals, selection)
    out = rf.emit(dev(m["vertices"]), dev(m["triangles"]), dev(m["colours"]))      # the allocating form
    assert raw(out["vertices"]) == exp[0].tobytes() and raw(out["colours"]) == exp[1].tobytes() and raw(out["triangles"]) == exp[3].tobytes()
    assert out["normals"] is None and out["selection"] is None


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_t", [255, 256, 257, 682, 683, 1365, 1366])
def test_triangle_counts_either_side_of_a_block_and_a_tile(rf, n_t):
    """3 n_t corners are 2 046, 2 049 (RUN_TILE) and 4 095, 4 098 (SORT_TILE); 256 is the block"""
    assert (RUN_TILE, SORT_TILE) == (2048, 4096) and 3 * 682 < RUN_TILE < 3 * 683 and 3 * 1365 < SORT_TILE < 3 * 1366
    soup = random_soup(120, n_t, n_t)
    c = assert_round(rf, case(soup, median_edge(soup)))
    assert min(c["k0"], c["k1"], c["k2"], c["k3"]) > 0
    assert_round(rf, case(soup, 0.0, np.arange(n_t) % 3 == 0))


def strip(n, seed):
    """n triangles in a row over n + 2 vertices: 2 n + 1 edges"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    pos = np.stack([0.5 * np.arange(n + 2), (np.arange(n + 2) % 2).astype(np.float64), np.zeros(n + 2)], 1) + rng.uniform(-0.1, 0.1, (n + 2, 3))
    return mesh(pos, np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1)))


def closed_fan(n, seed):
    """n triangles around the hub n: 2 n edges"""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(n) / n
    pos = np.concatenate([np.stack([np.cos(ang), np.sin(ang), rng.uniform(-0.1, 0.1, n)], 1), [[0.0, 0.0, 0.3]]])
    i = np.arange(n)
    return mesh(pos, np.stack([np.full(n, n), i, (i + 1) % n], 1))


@pytest.mark.parametrize("edges", [2047, 2048, 2049, 4095, 4096, 4097])
def test_edge_and_marked_counts_either_side_of_a_tile(rf, edges):
    """with L = 0 every edge is marked, so the edge scan, the compaction of the marks and the new vertices all end at the same count; then a
    length that marks the spokes of the fan or every second edge of the strip only"""
    m = closed_fan(edges // 2, edges) if edges % 2 == 0 else strip(edges // 2, edges)
    c = assert_round(rf, case(m, 0.0))
    assert c["edges"] == c["marked"] == edges and c["k3"] == len(m["triangles"])
    c = assert_round(rf, case(m, 0.9))
    assert 0 < c["marked"] < edges


@pytest.mark.parametrize("marked", [2047, 2048, 2049, 4095, 4096, 4097])
def test_marked_counts_either_side_of_a_tile_among_more_edges(rf, marked):
    """a strip of which only the first s triangles are selected has 2 s + 1 eligible edges, all marked with L = 0; a selected triangle that
    stands alone adds three, which makes the even counts"""
    s = (marked - 1) // 2 if marked % 2 else (marked - 4) // 2
    base = strip(s + 300, marked)
    n_v = len(base["vertices"])
    pos = np.concatenate([base["vertices"], np.array([(0, 50, 0), (1, 50, 0), (0, 51, 0)], F)])
    tri = np.concatenate([base["triangles"], np.array([(n_v, n_v + 1, n_v + 2)], U32)])
    sel = np.zeros(len(tri), U8)
    sel[:s] = 1
    sel[-1] = marked % 2 == 0
    c = assert_round(rf, case(mesh(pos, tri), 0.0, sel))
    assert c["marked"] == c["eligible"] == marked and c["edges"] > marked + 500, c


@pytest.mark.parametrize("n_v", [255, 256, 257, 65535, 65536, 65537])
def test_vertex_counts_either_side_of_a_sort_pass(rf, n_v):
    """the sentinel n_v of the sorts has 8, 9, 16 and 17 bits: one, two and three passes per round; a strip over the first vertices, a random
    soup over the largest indices, unreferenced vertices between"""
    rng = np.random.default_rng(n_v)
    st = strip(60, n_v)
    soup = rng.integers(n_v - 40, n_v, (300, 3))
    soup[-1] = (n_v - 1, n_v - 3, n_v - 2)
    pos = rng.uniform(-1, 1, (n_v, 3)).astype(F)
    pos[:62] = st["vertices"]
    c = assert_round(rf, case(mesh(pos, np.concatenate([st["triangles"], soup])), 0.8))
    assert c["marked"] > 0 and c["degenerate"] > 0


def test_a_hub_of_1024_and_an_edge_in_64(rf):
    fan = closed_fan(1024, 1)
    assert (fan["triangles"] == 1024).sum() == 1024
    c = assert_round(rf, case(fan, 0.5))                          # the 1 024 spokes
    assert c["marked"] == 1024 and c["k2"] == 1024
    rng = np.random.default_rng(64)
    pos = np.concatenate([[(0, 0, 0), (1, 0, 0)], rng.uniform(-1, 1, (64, 3)) + (0.5, 0, 0)])
    tri = np.stack([np.zeros(64, np.int64), np.ones(64, np.int64), 2 + np.arange(64)], 1)
    tri[1::2] = tri[1::2][:, (1, 0, 2)]
    table = RM.plan(tri, pos.astype(F), 0.99)
    assert (table["corner_edge"] == 0).sum() == 64 and table["rank"][0] == 0
    assert_round(rf, case(mesh(pos, tri), 0.99))


@pytest.mark.parametrize("seed", [1, 2])
def test_random_soups_of_20000(rf, seed):
    """duplicates, repeated indices and edges in dozens of triangles; L at the median edge, then half of it with every third triangle selected"""
    soup = with_attributes(random_soup(300, 20000, seed))
    L = median_edge(soup)
    c = assert_round(rf, case(soup, L), ((True, True, True), (False, False, False)))
    assert min(c["k0"], c["k1"], c["k2"], c["k3"]) > 1000 and c["degenerate"] > 50 and c["edges"] < 45000
    c = assert_round(rf, case(soup, 0.5 * L, (np.arange(20000) % 3 == 0) * 7))
    assert min(c["k1"], c["k2"], c["k3"]) > 0 and c["eligible"] < c["edges"]


# ---- life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_plans_and_emits_on_one_handle(ctx):
    """a handle of exactly the largest mesh's sizes: a smaller mesh after a larger one and back, empty ones in between; two emits on one
    plan; emit into exactly the result's rows and into one row fewer; the stage timing"""
    cases = all_cases()
    names = ("soup", "hand", "no_vertices", "soup", "cube_0.05", "no_triangles", "hand_selected", "grid_jitter", "soup")
    cap_v, cap_t = (max(len(cases[n][k]) for n in names) for k in ("vertices", "triangles"))
    h = RF.Refiner(ctx, cap_v, cap_t)
    try:
        with pytest.raises(ValueError):
            h.emit(dev(cases["hand"]["vertices"]), dev(cases["hand"]["triangles"]))          # nothing is planned
        to = torch.full((100, 3), -9, dtype=torch.int32, device="cuda")
        vo = torch.full((100, 3), -3.0, device="cuda")
        ctx.wait_torch_stream()
        with pytest.raises(Exception, match="rgbid error -1"):
            h.emit_into(dev(cases["hand"]["vertices"]), None, None, dev(cases["hand"]["triangles"]), None, vo, None, None, to, None)
        ctx.sync()
        assert (vo == -3.0).all() and (to == -9).all()
        for name in names:
            m = cases[name]
            assert_planned(h, m, planned(name))
            assert_emitted(h, m, emitted(name))
            assert_emitted(h, m, emitted(name), colours=False, selection=False)
        m, (ev, _, _, et, _) = cases["soup"], emitted("soup")
        vdev, tri = dev(m["vertices"]), dev(m["triangles"])
        assert len(ev) > len(m["vertices"]) and len(et) > len(m["triangles"])
        for dv, dt in ((1, 0), (0, 1)):
            vo, to = torch.full((len(ev), 3), -3.0, device="cuda"), torch.full((len(et), 3), -9, dtype=torch.int32, device="cuda")
            ctx.wait_torch_stream()
            with pytest.raises(Exception, match="rgbid error -1"):
                h.emit_into(vdev, None, None, tri, None, vo[:len(ev) - dv], None, None, to[:len(et) - dt], None)
            ctx.sync()
            assert (vo == -3.0).all() and (to == -9).all()
        with pytest.raises(ValueError):
            h.plan(tri, torch.zeros((cap_v + 1, 3), device="cuda"), 0.1)      # above the capacity
        h.timing(True)
        assert_planned(h, m, planned("soup"))
        assert_emitted(h, m, emitted("soup"))
        ms = h.timing(False)
        print("refine stage ms:", ms)
        assert tuple(ms) == RF.STAGES and all(np.isfinite(x) and x > 0 for x in ms.values())
    finally:
        h.close()


def test_refusals_and_reuse(rf):
    L = rf.L
    name = "soup"
    m, table = all_cases()[name], planned(name)
    sel = np.ones(len(m["triangles"]), U8)
    tri, vdev, cdev, ndev, sdev = dev(m["triangles"]), dev(m["vertices"]), dev(m["colours"]), dev(m["normals"]), dev(sel)
    n_v, n_t = len(m["vertices"]), len(m["triangles"])
    counts = (C.c_ulonglong * 9)()

    def still_works():
        assert_planned(rf, m, table)
        assert_emitted(rf, m, emitted(name))

    ev, ec, en, et, es = emitted(name)
    rows_v, rows_t = len(ev), len(et)
    vo, no = torch.zeros((rows_v + 1, 3), device="cuda"), torch.zeros((rows_v + 1, 3), device="cuda")
    co, to = torch.zeros((rows_v + 1, 3), dtype=torch.uint8, device="cuda"), torch.zeros((rows_t + 1, 3), dtype=torch.int32, device="cuda")
    so = torch.zeros((rows_t + 1,), dtype=torch.uint8, device="cuda")
    pv, pc, pn, pt, ps, pvo, pco, pno, pto, pso = (x.data_ptr() for x in (vdev, cdev, ndev, tri, sdev, vo, co, no, to, so))
    plan = lambda nv=n_v, nt=n_t, t=pt, v=pv, s=None, length=m["max_edge"]: L.rgbid_refine_plan(rf._h, nv, nt, t, v, s, length, counts)

    def emit(v=pv, c=pc, n=pn, t=pt, s=ps, vo=pvo, co=pco, no=pno, to=pto, so=pso, cv=rows_v, ct=rows_t):
        return L.rgbid_refine_emit(rf._h, v, c, n, t, s, vo, co, no, to, so, cv, ct)
    still_works()
    # a triangle that names a vertex that does not exist: the plan is refused, the former one is gone, the next one is right
    for where in (0, n_t // 2, n_t - 1):
        for value in (n_v, 0xFFFFFFFF):
            bad = np.array(m["triangles"], U32)
            bad[where, where % 3] = value
            with pytest.raises(Exception, match="rgbid error -1"):
                rf.plan(dev(bad), vdev, m["max_edge"])
            assert emit() == -1
        still_works()
    # the host-side refusals keep the plan: the emit after them is the former plan's
    for r in (lambda: plan(nv=CAP_V + 1), lambda: plan(nt=CAP_T + 1), lambda: plan(t=None), lambda: plan(t=pt + 1), lambda: plan(t=pt + 2),
              lambda: plan(nv=0), lambda: plan(v=None), lambda: plan(v=pv + 2), lambda: plan(length=-1e-300), lambda: plan(length=float("nan")),
              lambda: plan(length=float("inf")), lambda: plan(length=-float("inf"))):
        rf.ctx.wait_torch_stream()
        assert r() == -1
        assert_emitted(rf, m, emitted(name))
    for r in (lambda: emit(v=None), lambda: emit(t=None), lambda: emit(vo=None), lambda: emit(to=None), lambda: emit(c=None), lambda: emit(co=None),
              lambda: emit(n=None), lambda: emit(no=None), lambda: emit(s=None), lambda: emit(so=None), lambda: emit(v=pv + 2), lambda: emit(vo=pvo + 1),
              lambda: emit(n=pn + 2), lambda: emit(no=pno + 3), lambda: emit(t=pt + 2), lambda: emit(to=pto + 1), lambda: emit(cv=rows_v - 1),
              lambda: emit(ct=rows_t - 1), lambda: emit(vo=pv), lambda: emit(v=pvo), lambda: emit(v=pvo + 12), lambda: emit(to=pt),
              lambda: emit(t=pto + 12), lambda: emit(no=pn), lambda: emit(co=pc), lambda: emit(c=pco + 3), lambda: emit(so=ps), lambda: emit(s=pso + 1)):
        assert r() == -1
    rf.ctx.sync()
    assert not vo.any() and not co.any() and not no.any() and not to.any() and not so.any()
    assert raw(vdev) == m["vertices"].tobytes() and raw(tri) == m["triangles"].tobytes()
    assert emit() == 0
    rf.ctx.sync()
    assert raw(vo[:rows_v]) == ev.tobytes() and not vo[rows_v:].any() and raw(to[:rows_t]) == et.tobytes() and not to[rows_t:].any()
    assert raw(co[:rows_v]) == ec.tobytes() and raw(no[:rows_v]) == en.tobytes() and raw(so[:rows_t]) == es.tobytes() and not so[rows_t:].any()
    still_works()
    for bad in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError):                     # the Python checks come first
            rf.plan(tri, vdev, bad)
    with pytest.raises(ValueError):
        rf.plan(tri, vdev, 0.5, sdev[:-1])
    with pytest.raises(ValueError):
        rf.emit(vdev, tri, colours=cdev[:-1])
    with pytest.raises(ValueError):
        rf.emit(vdev, tri[:-1])
    with pytest.raises(ValueError):
        rf.emit(vdev, tri, selection=sdev[:-1])
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        with pytest.raises(Exception):
            RF.Refiner(rf.ctx, v, t)
    still_works()


# ---- the one-shot, the volume and the command line ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, rounds", [("cube_0.05", 4), ("cube_0.11", 4), ("cube_0.11", 2), ("fan_only", 4), ("hand", 0), ("soup_third", 3), ("no_triangles", 4)])
def test_one_shot_against_the_mirrors_rounds(ctx, name, rounds):
    m = all_cases()[name]
    ev, ec, et, en, es, figures = refined(name, rounds)
    sel = None if m["selection"] is None else dev(m["selection"])
    v, c, t, n, s, got = RF.refine_mesh(ctx, dev(m["vertices"]), dev(m["colours"]), dev(m["triangles"]), dev(m["normals"]), m["max_edge"], rounds, sel)
    assert raw(v) == ev.tobytes() and raw(c) == ec.tobytes() and raw(t) == et.tobytes() and raw(n) == en.tobytes()
    assert (s is None and m["selection"] is None) or raw(s) == es.tobytes()
    assert {k: got[k] for k in figures} == figures and got["vertices"] == len(ev) and got["triangles"] == len(et) and got["max_edge"] == m["max_edge"]
    if name == "cube_0.11":
        assert (got["left"] == 0) == (rounds == 4) and got["rounds_run"] == min(rounds, 3)


def test_volume_extract_refines_the_caps(ctx):
    """a sphere in 48^3 voxels with the weights of scattered voxels cleared, so that the surface has holes, through
    Volume.extract(fill_holes=..., refine={..., caps_only}, denoise=..., smooth=..., normals=True) against extract, then the mirrors: the
    filling, the split of the caps, the denoising, the smoothing and the normals of the last surface"""
    m = TM.Volume(48, 48, 48, (0.0, 0.0, 0.0), 0.05, 0.2)
    D, W = TM.sphere_state(m, (1.2, 1.2, 1.2), 0.9)
    W = W.copy()
    W.reshape(-1)[np.random.default_rng(11).choice(W.size, W.size // 300, replace=False)] = 0
    vol = TS.Volume(ctx, m.n, 1, colour=False)
    vol.configure(48, 48, 48, [0.0, 0.0, 0.0], 0.05, 0.2)
    vol.set_state(torch.from_numpy(D).cuda(), torch.from_numpy(W.view(np.int32)).cuda())
    host = [x.cpu().numpy() for x in vol.extract(1, normals=True)]
    host[2] = host[2].view(U32)
    fv, fc, ft, fn, filled = HM.fill(host[0], host[1], host[2], host[3], 32)
    sel = np.zeros(len(ft), U8)
    sel[len(host[2]):] = 1
    rv, rc, rt, rn, rs, figures = RM.refine(fv, fc, ft, fn, 0.03, 3, sel)
    assert filled["filled"] > 5 and figures["rounds_run"] >= 1 and len(rt) > len(ft)
    option = dict(max_edge=0.03, rounds=3, caps_only=True)
    v, c, t, n = vol.extract(1, normals=True, fill_holes=32, refine=option)
    got = vol.last_refine
    print("caps of a punched sphere:", {k: got[k] for k in ("rounds_run", "left", "vertices", "triangles")}, "from", len(fv), len(ft))
    assert raw(v) == rv.tobytes() and raw(t) == rt.tobytes() and raw(n) == rn.tobytes() and ((c is None and rc is None) or raw(c) == rc.tobytes())
    assert {k: got[k] for k in figures} == figures and vol.last_fill == filled
    ev, en, denoised, smoothed = mirrored_denoise(rv, rt, 2, dict(iterations=2))
    v, c, t, n = vol.extract(1, normals=True, fill_holes=32, refine=option, denoise=2, smooth=2)
    assert raw(v) == ev.tobytes() and raw(n) == en.tobytes() and raw(t) == rt.tobytes()
    assert vol.last_denoise == denoised and vol.last_smooth == smoothed
    # every triangle, a length alone
    av, ac, at, an, asel, afig = RM.refine(fv, fc, ft, fn, 0.06, 4)
    v, c, t = vol.extract(1, fill_holes=32, refine=0.06)[:3]
    assert raw(v) == av.tobytes() and raw(t) == at.tobytes() and {k: vol.last_refine[k] for k in afig} == afig and afig["rounds_run"] >= 1
    with pytest.raises(ValueError):
        vol.extract(1, refine=option)                              # caps_only without fill_holes
    vol.close()


def test_track_dataset_mesh_refine_option(ctx, tmp_path):
    """without the new option the PLY and the trajectory are what fuse gives today; with --mesh-refine the file holds exactly fuse's refined
    tensors, which are the mirrors', the trajectory and the mesh line are unchanged and one more line tells what the split did"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("refined", ["--mesh-normals", "--mesh-fill-holes", "32", "--mesh-refine", "0.04", "--mesh-refine-rounds", "2",
                                                   "--mesh-refine-caps"])):
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
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_refined.txt").read_bytes()
    v, c, t, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True)
    fv, fc, ft, fn, finfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True, normals=True,
                                    fill_holes=32)
    rv, rc, rt, rn, rinfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True, normals=True,
                                    fill_holes=32, refine=dict(max_edge=0.04, rounds=2, caps_only=True))
    assert (tmp_path / "plain.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0
    assert (tmp_path / "refined.ply").read_bytes() == TS.mesh_ply_bytes(rv, rc, rt, rn)
    sel = np.zeros(ft.shape[0], U8)
    sel[t.shape[0]:] = 1
    ev, ec, et, en, es, figures = RM.refine(fv.cpu().numpy(), fc.cpu().numpy(), ft.cpu().numpy().view(U32), fn.cpu().numpy(), 0.04, 2, sel)
    assert raw(rv) == ev.tobytes() and raw(rc) == ec.tobytes() and raw(rt) == et.tobytes() and raw(rn) == en.tobytes()
    f = rinfo["refine"]
    assert {k: f[k] for k in figures} == figures and "refine" not in info and "refine" not in finfo
    line = f"{info['voxels']} voxels of 0.05 m (truncation 0.2 m), {info['touched']} touched, {v.shape[0]} vertices, {t.shape[0]} triangles"
    assert line in said["plain"] and line in said["refined"] and "mesh refine" not in said["plain"]
    assert (f"mesh refine: edges above 0.04 m split in {f['rounds_run']} rounds, {sum(r['marked'] for r in f['rounds'])} new vertices, "
            f"{sum(r['new_triangles'] for r in f['rounds'])} new triangles, {f['left']} edges left above it") in said["refined"], said["refined"]
    mesh_lines = lambda s: [l.replace("refined.ply", "plain.ply") for l in s.splitlines() if " mesh of " in l]
    assert mesh_lines(said["plain"]) == mesh_lines(said["refined"]) and len(mesh_lines(said["plain"])) == 1
