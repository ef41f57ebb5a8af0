"""CPU checks of the states of tests/tsdf_states.py (counts at the cap of 65 535, colour sums that wrap, D that is NaN, infinite, a signed
zero, denormal or huge): that the states reach what the GPU tests need them to reach, asserted on the numpy mirrors alone; the mirrors
against the plain scalar loops of the contract on such states; and the values of include/rgbid_tsdf.h that can be worked out by hand."""
import functools

import numpy as np
import pytest

from tests import align_mirror as AM
from tests import raycast_mirror as RM
from tests import tsdf_mirror as TM
from tests import tsdf_states as S
from tests.render_mirror import NAN_BITS
from tests.test_cpu_consist import COLS, K, ROWS
from tests.test_cpu_tsdf import GATE, TH_GATE, TH_GRID, TH_K, mixed_scene, threshold_scene

F = np.float32
CAP = S.CAP
CAST = dict(z_min=0.3, z_max=5.0, step=0.05)
SMALL = dict(nx=7, ny=6, nz=5, origin=(-0.45, -0.35, 1.45), voxel=0.15, trunc=0.3)      # the grid of the scalar loops
KS = (15.0, 14.5, 7.5, 5.5)                                                             # the mixed scene's camera at a quarter of its size


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- what the states reach ------------------------------------------------------------------------------------------------------------
def test_saturated_state_reaches_the_caps_and_wraps():
    before = S.saturated_state()
    touched = S.clean_state().W > 0
    assert touched.sum() == 5189 and (before.W[touched] >= CAP - 5).all() and (before.Cn[touched] >= CAP - 5).all()
    assert not before.W[~touched].any() and (before.rgb[:, touched] >= (1 << 32) - 3000).all()
    assert set(np.unique(before.W[touched])) == set(np.unique(before.Cn[touched])) == set(range(CAP - 5, CAP + 1))
    assert ((before.Cn > before.W) & touched).any() and ((before.Cn < before.W) & touched).any()
    after = S.integrate(S.saturated_state(), S.views())
    grew = int((after.W[touched] > before.W[touched]).sum())
    reach = int(((before.W < CAP) & (after.W == CAP) & touched).sum())
    start = int((touched & (before.W == CAP)).sum())
    cn_reach = int(((before.Cn < CAP) & (after.Cn == CAP)).sum())
    cn_only = int(((after.Cn == CAP) & (after.W > before.W) & (before.Cn == CAP) & touched).sum())      # Cn capped while W grew
    wrapped = int((after.rgb < before.rgb).sum())
    unwrapped = int((after.rgb > before.rgb).sum())
    verts = len(TM.extract(after, CAP)[0])
    print(f"saturated: W grew in {grew}, reached the cap in {reach}, at the cap from the start {start}; Cn reached the cap in {cn_reach}, "
          f"was capped under a growing W in {cn_only}; {wrapped} sums wrapped, {unwrapped} grew; {verts} vertices at min_weight 65535")
    assert grew >= 2000 and reach >= 2000 and start >= 400 and cn_reach >= 500 and wrapped >= 1000 and verts >= 900
    assert cn_only >= 100 and unwrapped >= 1000
    assert after.W.max() == CAP and after.Cn.max() == CAP                                               # nothing carried past 16 bits
    at_cap = touched & (before.W == CAP)
    assert bits(after.D)[at_cap].tobytes() == bits(before.D)[at_cap].tobytes() and np.array_equal(after.rgb[:, at_cap], before.rgb[:, at_cap])
    # the min_weights of the GPU tests give three different meshes before the views (every W of 65 530 .. 65 535 is there) and large ones after
    assert len({TM.extract(before, mw)[0].tobytes() for mw in (1, CAP - 1, CAP)}) == 3 and len(TM.extract(before, CAP)[0]) >= 20
    assert all(len(TM.extract(after, mw)[0]) >= 900 for mw in (1, CAP - 1, CAP))


def cap_indices(count_of, vol, sc):
    """the view index at which every voxel's count (W or Cn) becomes 65 535 while the views of sc are integrated one by one: -> int64
    [nz, ny, nx], -1 where it was there before, V where it never gets there; and the voxels a view changed"""
    V = len(sc["R"])
    at = np.where(count_of(vol) == CAP, -1, V).astype(np.int64)
    changed = np.zeros(vol.shape, bool)
    for v in range(V):
        before = count_of(vol).copy()
        TM.integrate(vol, sc["planes"][v:v + 1], sc["colours"][v:v + 1], sc["R"][v:v + 1], sc["t"][v:v + 1], K, **GATE)
        changed |= count_of(vol) != before
        at[(at == V) & (count_of(vol) == CAP)] = v
    return at, changed


def test_cap_walk_reaches_the_cap_at_every_view_index():
    """W and Cn become 65 535 at every view index of the first launch (0 .. 15), at the first view of the second (16) and not at all, and
    every band holds voxels that a view really changes"""
    start = S.cap_walk_state()
    assert np.array_equal(np.unique(start.W), np.arange(CAP - 18, CAP + 1)) and np.array_equal(np.unique(start.Cn), np.arange(CAP - 18, CAP + 1))
    assert (start.Cn > start.W).any() and (start.Cn == start.W).any() and (start.Cn < start.W).any() and start.rgb.max() < 1 << 24
    for name, count_of in (("W", lambda v: v.W), ("Cn", lambda v: v.Cn)):
        at, changed = cap_indices(count_of, S.cap_walk_state(), S.views())
        hist = {v: int((at == v).sum()) for v in range(-1, S.VIEWS + 1)}
        band = [int((changed & (count_of(start) == CAP - k)).sum()) for k in range(1, S.WALK)]
        print(f"cap walk, {name}: voxels that reach the cap at view -1 (before) .. 17 (never): {list(hist.values())}; changed per band {band}")
        assert all(hist[v] >= 5 for v in range(S.VIEWS)), hist                          # every index of the first launch and index 16
        assert int(((at == S.VIEWS) & changed).sum()) >= 20                             # touched, and still below the cap
        assert min(band) >= 20
    after = S.integrate(S.cap_walk_state(), S.views())
    # in a band that was at the cap, the views change nothing at all; where only Cn was, W grows and the sums stay
    w_cap, cn_cap = start.W == CAP, (start.Cn == CAP) & (start.W < CAP)
    assert bits(after.D)[w_cap].tobytes() == bits(start.D)[w_cap].tobytes() and np.array_equal(after.counts()[w_cap], start.counts()[w_cap])
    assert np.array_equal(after.rgb[:, w_cap | cn_cap], start.rgb[:, w_cap | cn_cap]) and (after.W[cn_cap] > start.W[cn_cap]).sum() >= 20
    assert w_cap.sum() >= 20 and cn_cap.sum() >= 20 and after.W.max() == CAP and after.Cn.max() == CAP


@functools.lru_cache(maxsize=None)
def poisoned_results():
    vol, clean = S.poisoned_state(), S.clean_state()
    R, t = S.cast_views()
    planes, Ra, ta = S.align_views()
    return dict(vol=vol, mesh=TM.extract(vol, 1), edges=RM.active_edges(vol, 1), cast=RM.raycast(vol, R, t, K, ROWS, COLS, min_weight=1, **CAST),
                clean_cast=RM.raycast(clean, R, t, K, ROWS, COLS, min_weight=1, **CAST),
                align=AM.align(vol, planes, Ra, ta, K, ROWS, COLS, S.ALIGN_LEVELS, **GATE))


def test_poisoned_state_reaches_every_kind():
    r = poisoned_results()
    vol, (v, c, tri), (a, b, tt) = r["vol"], r["mesh"], r["edges"]
    assert set(vol.poison) == set(S.POISON) and all(len(i) >= 20 for i in vol.poison.values())
    nan = np.isnan(v)
    per_kind = {k: int((np.isin(a, i) | np.isin(b, i)).sum()) for k, i in vol.poison.items()}
    print(f"poisoned: {len(v)} vertices, {len(tri)} triangles, {int(nan.sum())} NaN components; active edges per kind {per_kind}")
    assert len(v) >= 2000 and len(tri) >= 4000 and nan.sum() >= 800 and min(per_kind.values()) >= 10
    assert (bits(v)[nan] == NAN_BITS).all()                                             # step 10: one bit pattern
    with np.errstate(all="ignore"):
        D = vol.D.reshape(-1)
        both_inf = np.isinf(D[a]) & np.isinf(D[b])
        assert both_inf.sum() >= 5 and np.isnan(tt[both_inf]).all()                     # inf / inf
        assert ((D[b] == 0) & np.isfinite(D[a])).sum() >= 10 and (tt[(D[b] == 0) & np.isfinite(D[a])] == 1).all()      # D_b = +-0: t = 1
        assert (np.isnan(D[b])).sum() >= 10 and not np.isnan(D[a]).any()                # a NaN is never the inside end
    cast, clean = r["cast"], r["clean_cast"]
    hit = np.isfinite(cast["depth"])
    nan_normal = hit & np.isnan(cast["normal"][:, 0])
    differs = bits(cast["depth"]) != bits(clean["depth"])
    print(f"poisoned: {int(hit.sum())} hits in 3 views, {int(nan_normal.sum())} with a NaN normal, {int(differs.sum())} depths differ from the clean state's")
    assert hit.sum() >= 500 and nan_normal.sum() >= 80 and differs.sum() >= 1000
    res = r["align"]
    print(f"poisoned: alignment status {res['status']}, iterations {res['iterations']}, used {res['used'].tolist()}")
    assert (res["iterations"] == sum(n for _, n in S.ALIGN_LEVELS)).all() and res["used"][:, 1].min() >= 64
    assert np.isfinite(res["sums"]).all() and np.isfinite(res["pose"]).all()            # |f| < trunc keeps what is not finite out


@pytest.mark.parametrize("alternate", [False, True])
def test_alignment_sums_take_a_nan_through_a_zero_fraction(alternate):
    vol, planes, R, t, a = S.align_nan_case(alternate)
    px = AM.pixel_values(vol, planes[0], AM.pose32(np.concatenate([R[0].reshape(9), t[0]])), TH_K, ROWS, COLS, 1, a["z_min"], a["z_max"],
                         a["min_weight"], a["huber"])
    J0, J5 = px["J"][0][:, 0], px["J"][5][:, 0]
    assert px["used"][:, 0].all() and (px["f"][:, 0] == 0).all()
    assert (np.isnan(J0).all() and np.isnan(J5).all()) if alternate else (np.isinf(J0).all() and np.isinf(J5).all())
    res = AM.align(vol, planes, R, t, TH_K, ROWS, COLS, **a)
    assert res["status"][0] == AM.SINGULAR and res["iterations"][0] == 1 and res["used"][0, 0] >= 64
    nan = np.isnan(res["sums"][0])
    assert nan.sum() >= 10 and not nan.all() and (res["sums"][0].view(np.uint64)[nan] == AM.NAN_BITS).all()        # step 33: one bit pattern
    assert res["pose"][0].tobytes() == np.concatenate([R[0].reshape(9), t[0]]).tobytes()
    assert res.tobytes() == AM.align_loop(vol, planes, R, t, TH_K, ROWS, COLS, **a).tobytes()


# ---- mirror against the scalar loops ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_states():
    """the 7 x 6 x 5 grid after the three views of mixed_scene(3), saturated and poisoned"""
    sc = mixed_scene(3)
    base = TM.integrate(TM.Volume(**SMALL), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)
    return S.saturate(S.clone(base), np.random.default_rng(5)), S.poison(S.clone(base), np.random.default_rng(6), 40, 1)


def assert_extract_equals_loop(vol, mw):
    v, c, tr = TM.extract(vol, mw)
    lv, lc, lt = TM.extract_loop(vol, mw)
    assert v.tobytes() == np.array(lv, F).reshape(-1, 3).tobytes() and c.tolist() == [list(x) for x in lc] and tr.tolist() == lt
    n = RM.vertex_normals(vol, mw)
    assert n.tobytes() == np.array(RM.normals_loop(vol, mw), F).reshape(-1, 3).tobytes() and len(n) == len(v)
    return v, c, tr


def test_mirror_equals_the_scalar_loop_on_saturated_counts():
    sat, _ = small_states()
    sc = S.views(without_colour=(3, 16))
    a = S.integrate(S.clone(sat), sc)
    b = TM.integrate_loop(S.clone(sat), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)
    assert a.state_bytes() == b.state_bytes()
    assert ((sat.W < CAP) & (a.W == CAP)).sum() >= 20 and ((sat.Cn < CAP) & (a.Cn == CAP)).sum() >= 10 and (a.rgb < sat.rgb).sum() >= 20
    for mw in (1, CAP - 1, CAP):
        v, c, tr = assert_extract_equals_loop(a, mw)
        assert len(v) > 10 and len(tr) > 10 and c.any()


def test_mirror_equals_the_scalar_loop_on_poisoned_values():
    _, poisoned = small_states()
    v, c, tr = assert_extract_equals_loop(poisoned, 1)                  # extract_loop used to raise on a NaN t
    assert np.isnan(v).sum() >= 10 and (bits(v)[np.isnan(v)] == NAN_BITS).all() and len(tr) > 20 and c.any()
    sc = S.views(0, 3)
    a = S.integrate(S.clone(poisoned), sc)
    b = TM.integrate_loop(S.clone(poisoned), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)
    assert a.state_bytes() == b.state_bytes() and (bits(a.D) != bits(poisoned.D)).sum() > 50
    assert_extract_equals_loop(a, 2)


def test_raycast_and_align_mirrors_equal_their_loops_on_the_states():
    R, t = S.cast_views()
    for vol, mw in ((S.poisoned_state(), 1), (S.integrate(S.saturated_state(), S.views()), CAP)):
        r = RM.raycast(vol, R[:2], t[:2], KS, 12, 16, min_weight=mw, **CAST)
        depth, normal, colour = RM.raycast_loop(vol, R[:2], t[:2], KS, 12, 16, min_weight=mw, **CAST)
        assert r["depth"].tobytes() == depth.tobytes() and r["normal"].tobytes() == normal.tobytes() and r["colour"].tobytes() == colour.tobytes()
        assert np.isfinite(depth).sum() >= 20 and colour.any()           # of 2 x 192 pixels
    assert (np.isfinite(depth) & np.isnan(normal[:, 0])).sum() == 0     # the saturated state is finite
    planes, Ra, ta = S.align_views()
    for vol, mw in ((S.poisoned_state(), 1), (S.integrate(S.saturated_state(), S.views()), CAP)):
        a = AM.align(vol, planes, Ra[:2], ta[:2], K, ROWS, COLS, ((4, 1), (2, 2)), min_pixels=16, min_weight=mw, **GATE)
        b = AM.align_loop(vol, planes, Ra[:2], ta[:2], K, ROWS, COLS, ((4, 1), (2, 2)), min_pixels=16, min_weight=mw, **GATE)
        assert a.tobytes() == b.tobytes() and (a["iterations"] == 3).all() and (a["used"] >= 16).all(), (a["iterations"], a["used"])


# ---- by hand --------------------------------------------------------------------------------------------------------------------------
def test_a_full_weight_takes_nothing_and_a_full_colour_count_lets_the_weight_grow():
    sc = threshold_scene()
    one = lambda vol: TM.integrate(vol, sc["planes"][:1], sc["colours"][:1], sc["R"][:1], sc["t"][:1], TH_K, **TH_GATE)
    mid = (4, 6, 8)                                        # the voxel at (0, 0, 2): view 0 measures s = 0 there
    r, g, b = (int(x) for x in sc["colours"][0][24, 32])
    v = one(TM.Volume(**TH_GRID))
    assert v.W[mid] == 1 and v.Cn[mid] == 1 and v.rgb[:, mid[0], mid[1], mid[2]].tolist() == [r, g, b]
    v = TM.Volume(**TH_GRID)                               # W = 65 535: untouched, whatever Cn is
    v.D[mid], v.W[mid], v.Cn[mid], v.rgb[:, 4, 6, 8] = F(0.0625), CAP, 7, (10, 20, 30)
    one(v)
    assert v.D[mid] == F(0.0625) and v.W[mid] == CAP and v.Cn[mid] == 7 and v.rgb[:, 4, 6, 8].tolist() == [10, 20, 30]
    v = TM.Volume(**TH_GRID)                               # W = 65 534 takes the last view: D = (D 65 534 + 0) / 65 535
    v.D[mid], v.W[mid], v.Cn[mid] = F(0.0625), CAP - 1, CAP - 1
    one(v)
    assert v.D[mid] == F(F(0.0625) * F(65534)) / F(65535) and v.W[mid] == CAP and v.Cn[mid] == CAP
    v = TM.Volume(**TH_GRID)                               # Cn = 65 535 and W = 5: W grows, the sums stop, no carry into W's half
    v.D[mid], v.W[mid], v.Cn[mid], v.rgb[:, 4, 6, 8] = F(0.0625), 5, CAP, (10, 20, 30)
    one(v)
    assert v.D[mid] == F(F(0.0625) * F(5)) / F(6) and v.W[mid] == 6 and v.Cn[mid] == CAP and v.rgb[:, 4, 6, 8].tolist() == [10, 20, 30]
    assert v.counts()[mid] == 0xFFFF0006
    v = TM.Volume(**TH_GRID)                               # step 8: the sums are modulo 2^32
    v.W[mid], v.Cn[mid], v.rgb[:, 4, 6, 8] = 1, 1, ((1 << 32) - 1, (1 << 32) - 256, 0)
    one(v)
    assert v.rgb[:, 4, 6, 8].tolist() == [(r - 1) % (1 << 32), (g - 256) % (1 << 32), b] and v.Cn[mid] == 2


def cell_volume(D, rgb=None, Cn=0):
    vol = TM.Volume(2, 2, 2, (0.0, 0.0, 0.0), 1.0, 1.0)
    vol.set_state(np.asarray(D, F).reshape(2, 2, 2), np.full((2, 2, 2), 1 | Cn << 16, np.uint32), rgb)
    return vol


def test_sign_decides_inside_to_the_last_denormal():
    for d0, inside in ((-0.0, False), (np.nan, False), (0.0, False), (1e-45, False), (-1e-45, True), (-1e-39, True), (-np.inf, True)):
        D = np.full(8, 0.5, F); D[0] = d0
        v, c, tr = TM.extract(cell_volume(D), 1)
        assert (len(v), len(tr)) == ((7, 6) if inside else (0, 0)), d0
        lv, lc, lt = TM.extract_loop(cell_volume(D), 1)
        assert (len(lv), len(lt)) == (len(v), len(tr))
    D = np.full(8, 0.5, F); D[0] = -1e-45
    v, _, _ = TM.extract(cell_volume(D), 1)
    assert (v == F(-1e-45) / (F(-1e-45) - F(0.5))).sum() == 12 and (v == 0).sum() == 9       # t is the denormals' quotient 2^-148, not 0


def test_zero_at_the_outside_end_keeps_its_zero_area_triangles():
    D = np.full(8, -0.5, F); D[7] = 0.0                    # seven corners inside, corner 7 at D_b = 0: every edge has t = 1
    v, c, tr = TM.extract(cell_volume(D), 1)
    assert len(v) == 7 and (v == 1).all() and len(tr) == 6 and len(np.unique(tr)) == 7
    assert TM.extract_loop(cell_volume(D), 1)[2] == tr.tolist()
    D[7] = -0.0                                            # -0.0 is outside as well
    assert TM.extract(cell_volume(D), 1)[0].tobytes() == v.tobytes()


def test_mean_of_the_largest_sum_and_colour_of_a_nan_t():
    rgb = np.zeros((3, 2, 2, 2), np.uint32)
    rgb[0] = (1 << 32) - 1; rgb[1] = 254; rgb[2, 0, 0, 0] = 100
    D = np.full(8, 0.5, F); D[0] = -0.5
    vol = cell_volume(D, rgb, 1)
    has, mean = TM._means(vol)
    assert has.all() and (mean[0] == 255).all() and (mean[1] == 254).all()       # (2 (2^32 - 1) + 1) / 2 = 2^32 - 1 -> 255: 64-bit arithmetic
    v, c, tr = TM.extract(vol, 1)
    assert (c == np.array([255, 254, 50], np.uint8)).all()
    D[0], D[1:] = -np.inf, np.inf                          # t = NaN: the positions are the one NaN, a mixed colour is 0
    vol = cell_volume(D, rgb, 1)
    v, c, tr = TM.extract(vol, 1)
    assert (bits(v) == NAN_BITS).all() and not c.any() and len(tr) == 6
    lv, lc, lt = TM.extract_loop(vol, 1)
    assert np.array(lv, F).tobytes() == v.tobytes() and not np.array(lc).any() and lt == tr.tolist()
