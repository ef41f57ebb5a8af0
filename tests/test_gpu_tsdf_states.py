"""GPU tests of the TSDF kernels (csrc/kernels_tsdf.hip) on the states of tests/tsdf_states.py, which no integration of clean data produces:
W and Cn at and next to the cap of 65 535, reached at every view index either side of the view chunk, colour sums that wrap modulo 2^32,
and D that is NaN, infinite, a signed zero, denormal or huge.  Every comparison is byte for byte against the numpy mirrors;
tests/test_cpu_tsdf_states.py asserts, on the mirrors alone, that the states reach what they are built for."""
import numpy as np
import pytest
import torch

from tests import align_mirror as AM
from tests import mesh_mirror as MM
from tests import raycast_mirror as RM
from tests import tsdf_mirror as TM
from tests import tsdf_states as S
from tests.render_mirror import NAN_BITS
from tests.test_cpu_consist import COLS, K, ROWS
from tests.test_cpu_raycast import ray_cameras
from tests.test_cpu_tsdf import GATE, TH_K, mixed_volume
from tests.test_gpu_align import assert_align
from tests.test_gpu_raycast import assert_cast, assert_normals, assert_planes, loaded
from tests.test_gpu_tsdf import assert_mesh, assert_state, both, upload

pytestmark = pytest.mark.gpu
F = np.float32
CAP = S.CAP
CAST = dict(z_min=0.3, z_max=5.0, step=0.05)
WEIGHTS = (1, CAP - 1, CAP)


def state_bytes(vol):
    return [x.cpu().numpy().tobytes() for x in vol.state()]


def assert_meshes(vol, mirror, weights=WEIGHTS):
    """vertices, colours, triangles and normals at every min_weight, and the vertices again without a colour buffer"""
    for mw in weights:
        ev, ec, et = assert_mesh(vol, mirror, mw)
        assert_normals(vol, mirror, mw)
        v, c, t = vol.extract(mw, colours=False)
        assert c is None and v.cpu().numpy().tobytes() == ev.tobytes() and t.cpu().numpy().view(np.uint32).tobytes() == et.tobytes()


@pytest.mark.parametrize("name", ["cap_walk", "saturated"])
def test_integrate_onto_counts_at_the_cap(ctx, name):
    """17 views in one call (the cap is reached inside the first launch's view loop, at the first view of the second launch, and not at
    all), the same 17 as the pieces (0, 1), (1, 16), (16, 17), then with views without colour in between"""
    make = getattr(S, name + "_state")
    sc = S.views()
    dplanes, dcols = upload(sc)
    mirror = make()
    vol = loaded(ctx, mirror)
    assert_state(vol, mirror)                              # set_state took the counts and sums as they are
    if name == "saturated":
        assert_meshes(vol, mirror)
    both(vol, mirror, sc, dplanes, dcols, sc["colours"], 0, S.VIEWS)
    assert_state(vol, mirror)
    one_call = state_bytes(vol)
    assert_meshes(vol, mirror)
    pieces = make()
    loaded(ctx, pieces, vol=vol)
    for a, b in ((0, 1), (1, 16), (16, 17)):
        both(vol, pieces, sc, dplanes, dcols, sc["colours"], a, b)
        assert_state(vol, pieces)
    assert state_bytes(vol) == one_call and list(pieces.state_bytes()) == one_call
    sc = S.views(without_colour=(0, 3, 15, 16))
    dplanes, dcols = upload(sc)
    fewer = make()
    loaded(ctx, fewer, vol=vol)
    both(vol, fewer, sc, dplanes, dcols, sc["colours"], 0, S.VIEWS)
    assert_state(vol, fewer)
    assert fewer.D.tobytes() == mirror.D.tobytes() and np.array_equal(fewer.W, mirror.W) and (fewer.Cn < mirror.Cn).sum() > 100
    assert_meshes(vol, fewer, (CAP,))
    vol.close()


def test_raycast_and_align_on_saturated_counts(ctx):
    """min_weight 65 535 is where ray_cell's running minimum starts, and Cn = 0xFFFF sits in the high half of every count it masks"""
    mirror = S.integrate(S.saturated_state(), S.views())
    vol = loaded(ctx, mirror)
    R, t = S.cast_views()
    planes, Ra, ta = S.align_views()
    hits = []
    for mw in (CAP, 1):
        want = assert_cast(vol, mirror, R, t, K, ROWS, COLS, min_weight=mw, **CAST)
        hits.append(int(np.isfinite(want["depth"]).sum()))
        assert hits[-1] > 500 and want["colour"].any()
        res = assert_align(ctx, vol, mirror, planes, Ra, ta, K, ROWS, COLS, levels=S.ALIGN_LEVELS, min_weight=mw, **GATE)
        assert (res["iterations"] >= 3).all() and (res["used"] >= 64).all()
    assert hits[0] < hits[1]                               # min_weight decides
    assert_cast(vol, mirror, R, t, K, ROWS, COLS, min_weight=CAP - 1, **CAST)
    vol.close()


def test_handle_without_colour_on_saturated_counts(ctx):
    """the Cn bits are in `counts` and there are no sums: meshes and views are black, the views leave Cn alone"""
    sat = S.saturated_state()
    plain = mixed_volume(colour=False)
    plain.set_state(sat.D, sat.counts())
    assert (plain.Cn >= CAP - 5).sum() == 5189
    vol = loaded(ctx, plain)
    assert_state(vol, plain)
    R, t = S.cast_views()
    for mw in (CAP, 1):
        ev, ec, et = assert_mesh(vol, plain, mw)
        assert len(ev) > 20 and not ec.any()
        want = assert_cast(vol, plain, R, t, K, ROWS, COLS, min_weight=mw, **CAST)
        assert not want["colour"].any()
    assert np.isfinite(want["depth"]).sum() > 500
    assert_state(vol, plain)                               # nothing was written
    sc = S.views()
    dplanes, dcols = upload(sc)
    cn = plain.Cn.copy()
    both(vol, plain, sc, dplanes, dcols, sc["colours"], 0, S.VIEWS)
    assert_state(vol, plain)
    assert np.array_equal(plain.Cn, cn) and plain.W.max() == CAP and (plain.W[cn > 0] == CAP).sum() > 2000
    vol.close()


def test_integrate_onto_poisoned_values(ctx):
    """step 7 on a D that is NaN (quiet, and signalling with a sign and a payload), infinite, denormal and huge"""
    mirror = S.poisoned_state()
    start = mirror.D.copy()
    vol = loaded(ctx, mirror)
    assert_state(vol, mirror)                              # the signalling NaN arrives as it is
    sc = S.views(0, 3)
    dplanes, dcols = upload(sc)
    both(vol, mirror, sc, dplanes, dcols, sc["colours"], 0, 3)
    was_nan, changed = np.isnan(start), start.view(np.uint32) != mirror.D.view(np.uint32)
    print("D after integrating onto a NaN, mirror:", sorted(hex(x) for x in set(mirror.D.view(np.uint32)[was_nan & changed].tolist())),
          "device:", sorted(hex(x) for x in set(vol.state()[0].cpu().numpy().view(np.uint32)[was_nan & changed].tolist())))
    assert (was_nan & changed).sum() >= 20 and np.isnan(mirror.D[was_nan]).all() and (changed & ~was_nan).sum() > 300
    assert_state(vol, mirror)
    assert_meshes(vol, mirror, (1, 2))
    vol.close()


def test_extract_and_filter_poisoned_values(ctx):
    mirror = S.poisoned_state()
    vol = loaded(ctx, mirror)
    for mw in (1, 2):
        ev, ec, et = assert_mesh(vol, mirror, mw)
        en = assert_normals(vol, mirror, mw)
        nan = np.isnan(ev)
        assert nan.sum() >= 400 and (ev.view(np.uint32)[nan] == NAN_BITS).all() and ec.any() and not np.isnan(en).any()
    # the component filter copies vertices as bytes: the NaN ones pass through unchanged
    table, _ = MM.label(et, len(ev))
    m = 50                                                 # the largest component and a few of dozens of triangles stay, the small ones go
    exp = MM.filter_mesh(et, len(ev), ev, ec, en, min_triangles=m)
    assert 0 < exp["components"] < len(table) and 0 < len(exp["triangles"]) < len(et)
    kept_nan = np.isnan(exp["vertices"])
    assert kept_nan.sum() >= 100 and (exp["vertices"].view(np.uint32)[kept_nan] == NAN_BITS).all()
    fv, fc, ft, fn = vol.extract(2, normals=True, min_component=m)
    assert fv.cpu().numpy().tobytes() == exp["vertices"].tobytes() and fc.cpu().numpy().tobytes() == exp["colours"].tobytes()
    assert ft.cpu().numpy().view(np.uint32).tobytes() == exp["triangles"].tobytes() and fn.cpu().numpy().tobytes() == exp["normals"].tobytes()
    assert vol.last_filter["kept_components"] == exp["components"] and vol.last_filter["components"] == len(table)
    vol.close()


def test_raycast_poisoned_values(ctx):
    mirror = S.poisoned_state()
    vol = loaded(ctx, mirror)
    R, t = S.cast_views()
    want = assert_cast(vol, mirror, R, t, K, ROWS, COLS, min_weight=1, **CAST)
    hit = np.isfinite(want["depth"])
    assert hit.sum() >= 500 and (hit & np.isnan(want["normal"][:, 0])).sum() >= 80 and ((want["hit_n"] >= 0) & ~hit).sum() >= 1
    for name in ("depth", "normal", "colour"):             # each output alone
        got = vol.raycast(R, t, K, ROWS, COLS, CAST["step"], 1, CAST["z_min"], CAST["z_max"], outputs=(name,))
        assert list(got) == [name] and got[name].cpu().numpy().tobytes() == want[name].tobytes(), name
    Rb, tb = (x[1:2] for x in ray_cameras(3))              # from behind, ragged tiles: exits beside NaN samples
    back = RM.raycast(mirror, Rb, tb, K, ROWS - 1, COLS - 1, min_weight=1, **CAST)
    got = vol.raycast(Rb, tb, K, ROWS - 1, COLS - 1, CAST["step"], 1, CAST["z_min"], CAST["z_max"])
    assert_planes(got, back)
    assert (back["exit_n"] >= 0).sum() > 300
    vol.close()


def test_align_poisoned_values(ctx):
    """the whole 560-byte records; |f| < trunc keeps every D that is not finite out of the sums ..."""
    mirror = S.poisoned_state()
    vol = loaded(ctx, mirror)
    planes, R, t = S.align_views()
    res = assert_align(ctx, vol, mirror, planes, R, t, K, ROWS, COLS, levels=S.ALIGN_LEVELS, **GATE)
    assert (res["iterations"] == 6).all() and res["used"][:, 1].min() >= 64 and np.isfinite(res["sums"]).all()
    vol.close()


@pytest.mark.parametrize("alternate", [False, True])
def test_align_sums_that_take_a_nan(ctx, alternate):
    """... but for a fraction of exactly 0 beside a huge D: J is infinite (or, with alternating signs, inf - inf), NaN enters the sums with
    the bits RGBID_TSDF_ALIGN_NAN_BITS and the view ends SINGULAR"""
    mirror, planes, R, t, a = S.align_nan_case(alternate)
    vol = loaded(ctx, mirror)
    res = assert_align(ctx, vol, mirror, planes, R, t, TH_K, ROWS, COLS, **a)
    nan = np.isnan(res["sums"][0])
    assert nan.sum() >= 10 and (res["sums"][0].view(np.uint64)[nan] == AM.NAN_BITS).all() and res["status"][0] == AM.SINGULAR
    vol.close()
