"""GPU tests of the hole-filling stage (include/rgbid_holes.h, csrc/kernels_holes.hip, rgbid.holes): the thirteen counts, the loop table
with its status and the emitted vertices, colours, normals and triangles byte for byte against the numpy restatement
(tests/holes_mirror.py) on the meshes of tests/test_cpu_holes.py, with and without each attribute, with both flags and max_edges of 3, 8, 64
and 2^31 - 1, canaries behind every output; loop lengths either side of a wave and of the tiles; a loop of 100 000 vertices (18 doubling
rounds, a serial sum whose value depends on its order); boundary half-edges, loops and filled loops either side of the tiles; vertex counts
either side of a change in the sort's pass count; plans, selections and emits in every order on one handle, exact capacities; every refusal;
and the options of rgbid.tsdf and tools/track_dataset.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import holes as HO, sequence, synth, tsdf as TS, tum
from tests import holes_mirror as HM
from tests import tsdf_mirror as TM
from tests.test_cpu_holes import all_cases, annulus, filled, mesh, permuted, selected, table_of
from tests.test_gpu_cloud import K_SMALL, write_tum_folder
from tests.test_gpu_simplify import chain
from tests.test_gpu_smooth import RUN_TILE, SORT_TILE, dev, full, mirrored_smooth, raw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32, U8 = np.float32, np.uint32, np.uint8
CAP_V, CAP_T = 600001, 200001
PAD = 3                                                     # rows behind every output that must keep their canary
ANY = (1 << 31) - 1


@pytest.fixture(scope="module")
def fl(ctx):
    """one handle for the whole file: every test after the first reuses it for a mesh of another size"""
    h = HO.Filler(ctx, CAP_V, CAP_T)
    yield h
    h.close()


def assert_planned(fl, tri, table):
    """the plan's counts, and the loop table in buffers with PAD canary rows behind them"""
    got = fl.plan(tri, table["n_v"])
    assert got == table["counts"], (got, table["counts"])
    n_l, s = table["counts"]["loops"], table["counts"]["loop_edges"]
    off, lv, lo = full(n_l + 1, (), torch.int32, -5), full(s, (), torch.int32, -6), full(s, (), torch.int32, -7)
    fl.ctx.wait_torch_stream()
    fl.loops_into(off, lv, lo, None, s)
    fl.ctx.sync()
    assert raw(off[:n_l + 1]) == table["offsets"].tobytes() and (off[n_l + 1:] == -5).all()
    assert raw(lv[:s]) == table["vertices"].tobytes() and (lv[s:] == -6).all()
    assert raw(lo[:s]) == table["owners"].tobytes() and (lo[s:] == -7).all()


def assert_selected(fl, vdev, table, sel, max_edges, any_facing):
    got = fl.select(vdev, max_edges, any_facing)
    assert got == sel["counts"], (max_edges, any_facing, got, sel["counts"])
    n_l = table["counts"]["loops"]
    st = full(n_l, (), torch.uint8, 0xA5)
    fl.ctx.wait_torch_stream()
    fl.loops_into(None, None, None, st, table["counts"]["loop_edges"])
    fl.ctx.sync()
    assert raw(st[:n_l]) == sel["status"].tobytes() and (st[n_l:] == 0xA5).all()


def assert_emitted(fl, m, exp, colours=True, normals=True):
    """one emit into buffers of exactly the rows of the result with PAD canary rows behind them: the bytes, the canaries, the inputs untouched"""
    ev, ec, en, et = exp
    ins = [dev(m["vertices"]), dev(m["colours"]) if colours else None, dev(m["normals"]) if normals else None, dev(m["triangles"])]
    before = [None if x is None else raw(x) for x in ins]
    rows_v, rows_t = len(ev), len(et)
    outs = [full(rows_v, (3,), torch.float32, 7.0), full(rows_v, (3,), torch.uint8, 0xA5) if colours else None,
            full(rows_v, (3,), torch.float32, -3.0) if normals else None, full(rows_t, (3,), torch.int32, -9)]
    cut = lambda x, rows: None if x is None else x[:rows]
    fl.ctx.wait_torch_stream()
    fl.emit_into(ins[0], ins[1], ins[2], ins[3], cut(outs[0], rows_v), cut(outs[1], rows_v), cut(outs[2], rows_v), cut(outs[3], rows_t))
    fl.ctx.sync()
    got_v, got_t = outs[0][:rows_v].cpu().numpy(), outs[3][:rows_t].cpu().numpy().view(U32)
    assert got_t.tobytes() == et.tobytes(), np.nonzero((got_t != et).any(1))[0][:10]
    assert got_v.tobytes() == ev.tobytes(), np.nonzero((got_v.view(U32) != ev.view(U32)).any(1))[0][:10]
    assert (outs[0][rows_v:] == 7.0).all() and (outs[3][rows_t:] == -9).all()
    if colours:
        assert raw(outs[1][:rows_v]) == ec.tobytes() and (outs[1][rows_v:] == 0xA5).all()
    if normals:
        assert raw(outs[2][:rows_v]) == en.tobytes() and (outs[2][rows_v:] == -3.0).all()
    assert [None if x is None else raw(x) for x in ins] == before


def assert_filled(fl, m, choices=((64, False), (64, True)), attributes=((True, True),)):
    """a mesh that is no case of the CPU file: plan, selections and emits against the mirror -> (table, the last selection)"""
    v = np.ascontiguousarray(m["vertices"], F)
    if m.get("colours") is None:
        rng = np.random.default_rng(len(v))
        m = dict(m, colours=rng.integers(0, 256, (len(v), 3), dtype=U8), normals=rng.normal(0, 1, (len(v), 3)).astype(F))
    table = HM.plan(m["triangles"], len(v))
    assert_planned(fl, dev(m["triangles"]), table)
    vdev = dev(v)
    for max_edges, any_facing in choices:
        sel = HM.select(table, v, max_edges, any_facing)
        assert_selected(fl, vdev, table, sel, max_edges, any_facing)
        exp = HM.emit(table, sel, v, m["colours"], m["normals"])
        for colours, normals in attributes:
            assert_emitted(fl, m, exp, colours, normals)
    return table, sel


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_cases_against_the_mirror(fl, name):
    m, table = all_cases()[name], table_of(name)
    tri, vdev = dev(m["triangles"]), dev(m["vertices"])
    assert_planned(fl, tri, table)
    for max_edges in (3, 8, 64, ANY):
        for any_facing in (False, True):
            sel = selected(name, max_edges, any_facing)
            assert_selected(fl, vdev, table, sel, max_edges, any_facing)
            exp = filled(name, max_edges, any_facing)
            for colours, normals in ((True, True), (False, False), (True, False), (False, True)) if max_edges == 64 else ((True, True),):
                assert_emitted(fl, m, exp, colours, normals)
    out = fl.emit(vdev, tri, dev(m["colours"]))                  # the allocating forms, on the last selection
    assert raw(out["vertices"]) == exp[0].tobytes() and raw(out["colours"]) == exp[1].tobytes() and raw(out["triangles"]) == exp[3].tobytes()
    assert out["normals"] is None
    got = fl.loops(status=True)
    assert raw(got["offsets"]) == table["offsets"].tobytes() and raw(got["vertices"]) == table["vertices"].tobytes()
    assert raw(got["owners"]) == table["owners"].tobytes() and raw(got["status"]) == sel["status"].tobytes()


def test_one_shot(ctx):
    m = all_cases()["sphere_40"]
    v, c, t, n, figures = HO.fill_holes(ctx, dev(m["vertices"]), None, dev(m["triangles"]), dev(m["normals"]), 16)
    ev, _, en, et = filled("sphere_40", 16)
    assert c is None and raw(v) == ev.tobytes() and raw(n) == en.tobytes() and raw(t) == et.tobytes()
    assert figures == dict(table_of("sphere_40")["counts"], **selected("sphere_40", 16)["counts"]) and figures["filled"] == 42


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097])
def test_loop_lengths_either_side_of_a_wave_and_the_tiles(fl, k):
    table, _ = assert_filled(fl, permuted(annulus(k), k), choices=((ANY, False), (ANY, True), (max(k - 1, 3), True)))
    assert table["counts"]["longest"] == k and table["counts"]["loops"] == 2


def test_a_loop_of_100000(fl):
    """200 000 simple vertices are 18 doubling rounds; the centre of the inner circle is one serial sum of 100 000 terms in which 1, 1e30 and
    -1e30 stand together: in loop order (0, k - 1, ..., 2, 1) they cancel last, in any other order the sum has other bits"""
    k = 100000
    m = annulus(k)
    m["vertices"][0:3, 0] = (1.0, 1e30, -1e30)
    table, sel = assert_filled(fl, m, choices=((ANY, False), (ANY, True)))
    assert table["counts"]["longest"] == k and int(2 * k).bit_length() == 18 and table["vertices"][:3].tolist() == [0, k - 1, k - 2]
    x = m["vertices"][table["vertices"][:k].astype(np.int64), 0].astype(np.float64)
    fwd = back = 0.0
    for a in x.tolist():
        fwd += a
    for a in x.tolist()[::-1]:
        back += a
    assert fwd != back and sel["centres"][0, 0] == F(fwd / k)


def sheet(w, h, holes, seed=0):
    """w x h quads, two triangles each, counter-clockwise from +z, without the quads (x, y) odd of the first `holes` of a seeded order: every
    one is a hole of 4, and the sheet's edge is one outline of 2 (w + h)"""
    x, y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    odd = np.flatnonzero((x % 2 == 1) & (y % 2 == 1) & (x < w - 1) & (y < h - 1))
    assert holes <= len(odd)
    keep = np.ones(len(x), bool)
    keep[np.random.default_rng(seed).permutation(odd)[:holes]] = False
    at = lambda i, j: i * (h + 1) + j
    a, b, c, d = at(x, y)[keep], at(x + 1, y)[keep], at(x + 1, y + 1)[keep], at(x, y + 1)[keep]
    gx, gy = np.meshgrid(np.arange(w + 1), np.arange(h + 1), indexing="ij")
    rng = np.random.default_rng(seed + 1)
    pos = np.stack([gx.reshape(-1) + rng.uniform(-0.2, 0.2, gx.size), gy.reshape(-1) + rng.uniform(-0.2, 0.2, gx.size), rng.uniform(-0.1, 0.1, gx.size)], 1)
    return permuted(mesh(pos, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])), seed)


@pytest.mark.parametrize("w, h, holes", [(47, 48, 464), (47, 47, 465), (47, 48, 465), (67, 68, 956), (67, 67, 957), (67, 68, 957),
                                         (131, 131, 2046), (131, 131, 2047), (131, 131, 2048), (131, 131, 2049),
                                         (131, 131, 4094), (131, 131, 4095), (131, 131, 4096), (131, 131, 4097)])
def test_half_edges_and_loops_either_side_of_a_tile(fl, w, h, holes):
    """n_b = 4 holes + 2 (w + h) is 2046, 2048, 2050 and 4094, 4096, 4098 on the small sheets; on the large ones L = holes + 1 and F = holes
    lie either side of 2048 and 4096"""
    assert (RUN_TILE, SORT_TILE) == (2048, 4096)
    table, sel = assert_filled(fl, sheet(w, h, holes, seed=holes), choices=((4, False),))
    c = table["counts"]
    assert c["boundary_half_edges"] == 4 * holes + 2 * (w + h) and c["loops"] == holes + 1 and c["blocked"] == 0
    assert sel["counts"] == dict(too_long=1, not_finite=0, outlines=0, filled=holes, new_triangles=4 * holes)
    if w < 131:
        assert c["boundary_half_edges"] in (RUN_TILE - 2, RUN_TILE, RUN_TILE + 2, SORT_TILE - 2, SORT_TILE, SORT_TILE + 2)


@pytest.mark.parametrize("n_v", [255, 256, 257, 65535, 65536, 65537])
def test_vertex_counts_either_side_of_a_sort_pass(fl, n_v):
    """the sentinel n_v of the sorts has 8, 9, 16 and 17 bits: one, two and three passes per round; an annulus over the first vertices, a
    random soup over the largest indices, unreferenced vertices between"""
    rng = np.random.default_rng(n_v)
    ring = permuted(annulus(40), n_v)
    soup = rng.integers(n_v - 40, n_v, (300, 3))
    soup[-1] = (n_v - 1, n_v - 3, n_v - 2)
    pos = rng.uniform(-1, 1, (n_v, 3)).astype(F)
    pos[:80] = ring["vertices"]
    table, sel = assert_filled(fl, mesh(pos, np.concatenate([ring["triangles"], soup])), choices=((64, False), (64, True)))
    assert table["counts"]["loops"] >= 2 and table["counts"]["non_simple"] > 0 and sel["counts"]["filled"] >= 2


# ---- life cycle ------------------------------------------------------------------------------------------------------------------------------
def test_plans_selections_and_emits_on_one_handle(ctx):
    """a handle of exactly the largest mesh's sizes: a smaller mesh after a larger one and back, no vertices in between; two selections and
    emits on one plan; emit and the status without a selection; emit into exactly the result's rows and into one row fewer"""
    cases = all_cases()
    names = ("noise", "hand", "no_vertices", "noise", "sphere_40", "no_triangles", "hand", "annulus_2048_permuted", "noise")
    cap_v, cap_t = (max(len(cases[n][k]) for n in names) for k in ("vertices", "triangles"))
    h = HO.Filler(ctx, cap_v, cap_t)
    try:
        for name in names:
            m, table = cases[name], table_of(name)
            tri, vdev = dev(m["triangles"]), dev(m["vertices"])
            assert_planned(h, tri, table)
            rows_v, rows_t = len(m["vertices"]) + 1, len(m["triangles"]) + 3
            vo, to = torch.full((rows_v, 3), -3.0, device="cuda"), torch.full((rows_t, 3), -9, dtype=torch.int32, device="cuda")
            st = torch.full((table["counts"]["loops"] + 1,), 0xA5, dtype=torch.uint8, device="cuda")
            ctx.wait_torch_stream()
            with pytest.raises(ValueError):
                h.emit(vdev, tri)                                     # nothing is selected
            with pytest.raises(Exception, match="rgbid error -1"):
                h.emit_into(vdev, None, None, tri, vo, None, None, to)
            with pytest.raises(Exception, match="rgbid error -1"):
                h.loops_into(None, None, None, st, table["counts"]["loop_edges"])
            ctx.sync()
            assert (vo == -3.0).all() and (to == -9).all() and (st == 0xA5).all()
            for max_edges, any_facing in ((8, True), (64, False)):   # the second selection replaces the first
                assert_selected(h, vdev, table, selected(name, max_edges, any_facing), max_edges, any_facing)
                assert_emitted(h, m, filled(name, max_edges, any_facing))
                assert_emitted(h, m, filled(name, max_edges, any_facing), colours=False)
        ev, _, _, et = filled("noise")
        assert len(ev) > len(cases["noise"]["vertices"]) and len(et) > len(cases["noise"]["triangles"])
        for dv, dt in ((1, 0), (0, 1)):
            vo, to = torch.full((len(ev), 3), -3.0, device="cuda"), torch.full((len(et), 3), -9, dtype=torch.int32, device="cuda")
            ctx.wait_torch_stream()
            with pytest.raises(Exception, match="rgbid error -1"):
                h.emit_into(vdev, None, None, tri, vo[:len(ev) - dv], None, None, to[:len(et) - dt])
            ctx.sync()
            assert (vo == -3.0).all() and (to == -9).all()
        with pytest.raises(ValueError):
            h.plan(tri, cap_v + 1)                                    # above the capacity
        h.timing(True)
        assert_planned(h, tri, table)
        assert_selected(h, vdev, table, selected("noise"), 64, False)
        assert_emitted(h, m, filled("noise"))
        ms = h.timing(False)
        print("holes stage ms:", ms)
        assert tuple(ms) == HO.STAGES and all(np.isfinite(x) and x > 0 for x in ms.values())
    finally:
        h.close()


def test_refusals_and_reuse(fl):
    L = fl.L
    name = "sphere_40"
    m, table = all_cases()[name], table_of(name)
    tri, vdev, cdev, ndev = dev(m["triangles"]), dev(m["vertices"]), dev(m["colours"]), dev(m["normals"])
    n_v, n_t = len(m["vertices"]), len(m["triangles"])
    counts, chosen = (C.c_ulonglong * 8)(), (C.c_ulonglong * 5)()

    def still_works():
        assert_planned(fl, tri, table)
        assert_selected(fl, vdev, table, selected(name, 16), 16, False)
        assert_emitted(fl, m, filled(name, 16))

    ev, ec, en, et = filled(name, 16)
    rows_v, rows_t, s = len(ev), len(et), table["counts"]["loop_edges"]
    vo, no = torch.zeros((rows_v + 1, 3), device="cuda"), torch.zeros((rows_v + 1, 3), device="cuda")
    co, to = torch.zeros((rows_v + 1, 3), dtype=torch.uint8, device="cuda"), torch.zeros((rows_t + 1, 3), dtype=torch.int32, device="cuda")
    buf = torch.zeros(2 * s + 100, dtype=torch.int32, device="cuda")
    pv, pc, pn, pt, pvo, pco, pno, pto, pb = (x.data_ptr() for x in (vdev, cdev, ndev, tri, vo, co, no, to, buf))
    plan = lambda nv=n_v, nt=n_t, t=pt: L.rgbid_holes_plan(fl._h, nv, nt, t, counts)
    select = lambda v=pv, k=16, flags=0: L.rgbid_holes_select(fl._h, v, k, flags, chosen)
    loops = lambda off=pb, lv=None, lo=None, st=None, cap=s: L.rgbid_holes_loops(fl._h, off, lv, lo, st, cap)

    def emit(v=pv, c=pc, n=pn, t=pt, vo=pvo, co=pco, no=pno, to=pto, cv=rows_v, ct=rows_t):
        return L.rgbid_holes_emit(fl._h, v, c, n, t, vo, co, no, to, cv, ct)
    still_works()
    # a triangle that names a vertex that does not exist: the plan is refused, the former one is gone, the next one is right
    for where in (0, n_t // 2, n_t - 1):
        for value in (n_v, 0xFFFFFFFF):
            bad = np.array(m["triangles"], U32)
            bad[where, where % 3] = value
            with pytest.raises(Exception, match="rgbid error -1"):
                fl.plan(dev(bad), n_v)
            assert select() == -1 and loops() == -1 and emit() == -1
        still_works()
    # the host-side refusals keep the plan and the selection: the calls after them are the former plan's
    for r in (lambda: plan(nv=CAP_V + 1), lambda: plan(nt=CAP_T + 1), lambda: plan(t=None), lambda: plan(t=pt + 1), lambda: plan(t=pt + 2),
              lambda: plan(nv=0), lambda: select(k=2), lambda: select(k=0), lambda: select(k=1 << 31), lambda: select(k=0xFFFFFFFF),
              lambda: select(flags=2), lambda: select(flags=0x80000001), lambda: select(v=None), lambda: select(v=pv + 2)):
        fl.ctx.wait_torch_stream()
        assert r() == -1
        assert_emitted(fl, m, filled(name, 16))
    for r in (lambda: emit(v=None), lambda: emit(t=None), lambda: emit(vo=None), lambda: emit(to=None), lambda: emit(c=None), lambda: emit(co=None),
              lambda: emit(n=None), lambda: emit(no=None), lambda: emit(v=pv + 2), lambda: emit(vo=pvo + 1), lambda: emit(n=pn + 2),
              lambda: emit(no=pno + 3), lambda: emit(t=pt + 2), lambda: emit(to=pto + 1), lambda: emit(cv=rows_v - 1), lambda: emit(ct=rows_t - 1),
              lambda: emit(vo=pv), lambda: emit(v=pvo), lambda: emit(v=pvo + 12), lambda: emit(to=pt), lambda: emit(t=pto + 12), lambda: emit(no=pn),
              lambda: emit(co=pc), lambda: emit(c=pco + 3),
              lambda: loops(cap=s - 1), lambda: loops(off=pb + 2), lambda: loops(lv=pb + 1), lambda: loops(lo=pb + 3)):
        assert r() == -1
    fl.ctx.sync()
    assert not vo.any() and not co.any() and not no.any() and not to.any() and not buf.any()
    assert raw(vdev) == m["vertices"].tobytes() and raw(tri) == m["triangles"].tobytes()
    assert emit() == 0 and loops() == 0
    fl.ctx.sync()
    assert raw(vo[:rows_v]) == ev.tobytes() and not vo[rows_v:].any() and raw(to[:rows_t]) == et.tobytes() and not to[rows_t:].any()
    assert raw(co[:rows_v]) == ec.tobytes() and raw(no[:rows_v]) == en.tobytes()
    assert raw(buf[:len(table["offsets"])]) == table["offsets"].tobytes() and not buf[len(table["offsets"]):].any()
    still_works()
    for bad in (2, 1 << 31, 8.0):
        with pytest.raises(ValueError):                     # the Python checks come first
            fl.select(vdev, bad)
    with pytest.raises(ValueError):
        fl.select(vdev[:-1])
    with pytest.raises(ValueError):
        fl.emit(vdev, tri, colours=cdev[:-1])
    with pytest.raises(ValueError):
        fl.emit(vdev, tri[:-1])
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        with pytest.raises(Exception):
            HO.Filler(fl.ctx, v, t)
    still_works()


# ---- through the volume, a tracked run and the command line -----------------------------------------------------------------------------
def mirrored_fill(v, c, t, n, **kw):
    kw = HO.fill_holes_arg(kw)
    return HM.fill(v, c, t, n, kw["max_edges"], kw["any_facing"])


def test_volume_extract_fills_holes(ctx):
    """a large and a small sphere in 128 x 64 x 64 voxels with the weights of scattered voxels cleared, so that the surface has holes,
    through Volume.extract(min_component=..., simplify=..., fill_holes=..., smooth=..., normals=True) against extract, then the mirrors:
    fragments first, then decimation, then the filling, then smoothing with the normals of the smoothed surface"""
    m = TM.Volume(128, 64, 64, (0.0, 0.0, 0.0), 0.05, 0.2)
    big, W = TM.sphere_state(m, (3.2, 1.6, 1.6), 1.5)
    small, _ = TM.sphere_state(m, (0.4, 0.4, 0.4), 0.25)
    W = W.copy()
    W.reshape(-1)[np.random.default_rng(11).choice(W.size, W.size // 400, replace=False)] = 0
    vol = TS.Volume(ctx, m.n, 1, colour=False)
    vol.configure(128, 64, 64, [0.0, 0.0, 0.0], 0.05, 0.2)
    vol.set_state(torch.from_numpy(np.minimum(big, small)).cuda(), torch.from_numpy(W.view(np.int32)).cuda())
    host = [x.cpu().numpy() for x in vol.extract(1, normals=True)]
    host[2] = host[2].view(U32)
    # the filling alone
    fv, fc, ft, fn, figures = mirrored_fill(host[0], host[1], host[2], host[3], max_edges=32)
    v, c, t, n = vol.extract(1, normals=True, fill_holes=32)
    print("punched spheres:", figures)
    assert figures["filled"] > 20 and vol.last_fill == figures
    assert raw(v) == fv.tobytes() and raw(t) == ft.tobytes() and raw(n) == fn.tobytes() and ((c is None and fc is None) or raw(c) == fc.tobytes())
    # the whole chain
    exp, info, _ = chain(*host, 0.2, min_triangles=5000)
    fv, fc, ft, fn, figures = mirrored_fill(exp["vertices"], exp["colours"], exp["triangles"], exp["normals"], max_edges=64, any_facing=True)
    ev, en, smoothed = mirrored_smooth(fv, ft, iterations=5)
    v, c, t, n = vol.extract(1, normals=True, min_component=5000, simplify=0.2, fill_holes=dict(max_edges=64, any_facing=True), smooth=5)
    assert vol.last_fill == figures and vol.last_simplify == info and vol.last_smooth == smoothed
    assert raw(v) == ev.tobytes() and raw(n) == en.tobytes() and raw(t) == ft.tobytes()
    vol.close()


def test_fuse_fills_a_tracked_run(ctx):
    """the tracked run of tests/test_gpu_tsdf.py through fuse(fill_holes=64) against fuse, then the mirror.  The figures are printed and
    asserted against the mirror only (DESIGN.md section 30 holds the measured ones)."""
    rows, cols, n = 120, 160, 24
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", noise=False, dropout=0.0, trans_step=(0.01, 0.02),
                              rot_step_deg=(0.5, 1.0))
    depth, rgb = seq["depth"].to(torch.int16).contiguous(), seq["rgb"].contiguous()
    _, _, _, pc = sequence.track_chunked(ctx, depth, rgb, 2, K_SMALL, cloud="novel", visratio_odo=0.985, visratio_integr=0.97, keyframe_depth=True,
                                         keyframe_colour=True)
    v, c, t, nrm, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, normals=True)
    assert "fill_holes" not in info
    fv, fc, ft, fn, finfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.04, points=pc.points, return_volume=True, normals=True, fill_holes=64)
    ev, ec, et, en, figures = mirrored_fill(v.cpu().numpy(), c.cpu().numpy(), t.cpu().numpy().view(U32), nrm.cpu().numpy(), max_edges=64)
    print("tracked run:", finfo["fill_holes"], "of", v.shape[0], "vertices,", t.shape[0], "triangles")
    assert finfo["fill_holes"] == figures and {k: finfo[k] for k in info} == info
    assert raw(fv) == ev.tobytes() and raw(fc) == ec.tobytes() and raw(ft) == et.tobytes() and raw(fn) == en.tobytes()


def test_track_dataset_mesh_fill_holes_option(ctx, tmp_path):
    """without the new option the PLY and the trajectory are what fuse gives today; with --mesh-fill-holes the file holds exactly fuse's
    filled tensors, the trajectory and the mesh line are unchanged and one more line tells what the filling did"""
    rows, cols, n = 120, 160, 30
    seq = synth.make_sequence(n, K=K_SMALL, rows=rows, cols=cols, device="cuda", trans_step=(0.02, 0.04), rot_step_deg=(1.0, 2.0))
    root = tmp_path / "synth"
    write_tum_folder(root, seq)
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    base = [sys.executable, tool, str(root), "--rows", str(rows), "--cols", str(cols), "--K"] + [repr(float(v)) for v in K_SMALL] + ["--chunks", "2"]
    said = {}
    for name, extra in (("plain", []), ("filled", ["--mesh-normals", "--mesh-fill-holes", "32", "--mesh-fill-any-facing"])):
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
    assert (tmp_path / "traj_plain.txt").read_bytes() == (tmp_path / "traj_filled.txt").read_bytes()
    v, c, t, info = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True)
    fv, fc, ft, fn, finfo = TS.fuse(ctx, pc.keyframes, K_SMALL, rows, cols, voxel=0.05, min_weight=2, points=pc.points, return_volume=True, normals=True,
                                    fill_holes=dict(max_edges=32, any_facing=True))
    assert (tmp_path / "plain.ply").read_bytes() == TS.mesh_ply_bytes(v, c, t) and t.shape[0] > 0
    assert (tmp_path / "filled.ply").read_bytes() == TS.mesh_ply_bytes(fv, fc, ft, fn) and raw(ft[:t.shape[0]]) == raw(t)
    line = f"{info['voxels']} voxels of 0.05 m (truncation 0.2 m), {info['touched']} touched, {v.shape[0]} vertices, {t.shape[0]} triangles"
    assert line in said["plain"] and line in said["filled"] and "mesh fill holes" not in said["plain"]
    f = finfo["fill_holes"]
    assert (f"mesh fill holes: {f['loops']} loops, {f['filled']} filled, {f['outlines']} outlines, {f['too_long']} too long, {f['blocked']} blocked "
            f"half-edges, {f['new_triangles']} new triangles") in said["filled"], said["filled"]
    mesh_lines = lambda s: [l.replace("filled.ply", "plain.ply") for l in s.splitlines() if " mesh of " in l]
    assert mesh_lines(said["plain"]) == mesh_lines(said["filled"]) and len(mesh_lines(said["plain"])) == 1
